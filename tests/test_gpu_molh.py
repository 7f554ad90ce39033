"""-m gpu: mdt_mol_hydrogens (csrc/k_molh.hip), mol_hydrogens(), mol_formula() and the screening call with ``kekulize`` on the
device.  Every comparison is exact: hydrogens, partners, verdict, atom and formula against the plain-int reference tests/molh_ref.py
(whose graphs are tests/molkey_ref.py's).  No row here can run longer than its step cap: at most 4096 tries a row."""
import random

import numpy as np
import pytest
import torch

import molh_ref as H
import molkey_ref as K
import smiles_ref as S
from gpu_util import DEV, make_model
from test_molh_host import BACKTRACK, NO_MOLECULE, TABLE, respelled_table
from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, formula_strings, mol_formula, mol_hydrogens, mol_weight,
                                              runtime as rt, screen_tokens_diverse)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

RING_MAX = "c" + "0123456789" + ("c" + "0123456789" * 2) * 2 + "c" + "0123456789"     # 64 tokens, 4 atoms, 30 ring bonds
AROMATIC_64 = "c%10ccc(cc%10)c%11ccc(cc%11)c%12ccc(cc%12)c%13ccc(cc%13)c1ccccc1"      # 64 tokens, five rings in a row
ROWS_PER_BLOCK = 4                                                          # k_mol_hydrogens: waves (rows) of a workgroup


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()[:120]


@pytest.fixture(scope="module")
def pool(spelled):
    """Strings of at most 64 tokens: the table and its respellings, random spellings, rows that are no molecule."""
    rows = TABLE + [t for _, sp in respelled_table(random.Random(3)) for t in sp] + [s for _, sp in spelled for s in sp]
    rows += NO_MOLECULE + [s[:64] for s in S.mutated_rows(128)]
    assert all(len(s) <= 64 for s in rows) and sum(H.string_hydrogens(s)["verdict"] == 2 for s in rows) > 20
    return rows


@pytest.fixture(scope="module")
def vocab(pool):
    return SmilesVocabulary([None] + sorted(set(S.CHARS) | set("".join(pool)) | set("$:*%\\/csnopbBPSI")))


def graph_arrays(strings, vocabulary, width):
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    return torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]


def agree_arrays(got, want, what=None):
    """got: the five tensors of the op; want: the reference's rows."""
    torch.cuda.synchronize()
    hydrogens, partner, verdict, atom, formula = got
    assert (hydrogens.dtype, partner.dtype, verdict.dtype, atom.dtype, formula.dtype) == (torch.uint8,) * 3 + (torch.int32,) * 2
    assert verdict.tolist() == [r["verdict"] for r in want], what
    assert atom.tolist() == [r["atom"] for r in want], what
    assert hydrogens.tolist() == [r["hydrogens"] for r in want], what
    assert partner.tolist() == [r["partner"] for r in want], what
    assert formula.tolist() == [r["formula"] for r in want], what


def agree(strings, vocabulary, L, cap=H.MAX_STEPS, what=None):
    want = [H.string_hydrogens(s, cap, L) for s in strings]
    agree_arrays(torch.ops.mdt.mol_hydrogens(*graph_arrays(strings, vocabulary, L), cap), want, what)
    return want


def test_the_table_and_the_spelling_pool_through_the_op_and_the_public_calls(pool, vocab):
    want = agree(pool, vocab, 64, what="pool")
    assert {r["verdict"] for r in want} == {0, 1, 2}
    ids = vocab.encode(pool, 64)
    hydrogens, partner, verdict, atom, status, position = mol_hydrogens(ids, vocab, DEV)
    counts, verdict2, status2, position2 = mol_formula(ids.to(torch.int16), vocab, DEV)
    torch.cuda.synchronize()
    assert all(t.dtype == torch.int64 for t in (hydrogens, partner, verdict, atom, status, position, counts, verdict2))
    assert hydrogens.tolist() == [r["hydrogens"] for r in want] and partner.tolist() == [r["partner"] for r in want]
    assert verdict.tolist() == verdict2.tolist() == [r["verdict"] for r in want] and atom.tolist() == [r["atom"] for r in want]
    assert counts.tolist() == [r["formula"] for r in want]
    assert status.tolist() == status2.tolist() == [S.check(s)[0] for s in pool] and torch.equal(position, position2)
    assert formula_strings(counts) == [H.formula_string(r["formula"]) for r in want]
    by = dict(zip(pool, formula_strings(counts)))
    assert by["c1ccccc1"] == "C6H6" and by["Cn1cnc2c1c(=O)n(C)c(=O)n2C"] == "C8H10N4O2" and by["[NH4+]"] == "H4N+" and by["C("] == ""
    assert abs(float(mol_weight(counts)[pool.index("CCO")]) - 46.069) < 2e-3
    for g, sp in respelled_table(random.Random(3)):                          # the verdict does not depend on the spelling
        assert len({int(verdict[pool.index(t)]) for t in sp + [g]}) == 1, g


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 67])
@pytest.mark.parametrize("L", [1, 33, 64])
def test_row_shapes(L, R_, pool, vocab):
    """Molecule rows interleaved with empty rows and rows of status != 0, cut to the width (some become no molecule: a case)."""
    rng = np.random.default_rng(100 * L + R_)
    if L == 1:
        strings = [["c", "C", "*", "", "(", "n", "F", "s"][int(rng.integers(8))] for _ in range(R_)]
    else:
        strings = [["", "C(", pool[int(rng.integers(len(pool)))][:L]][min(int(rng.integers(6)), 2)] for _ in range(R_)]
    agree(strings, vocab, L, what=(L, R_))


def test_no_rows_launches_nothing(vocab):
    empty = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV)
    out = torch.ops.mdt.mol_hydrogens(empty[0], empty[1], empty[0], empty[1], 4096)
    assert [tuple(t.shape) for t in out] == [(0, 8), (0, 8), (0,), (0,), (0, 13)]
    assert mol_hydrogens(torch.zeros(0, 8, dtype=torch.long), vocab, DEV)[0].shape == (0, 8)


def test_full_width_rows(vocab):
    strings = [AROMATIC_64, "C" * 64, "c" * 64, RING_MAX, RING_MAX.replace("c", "*"), "c1ccccc1" * 8, "*" * 64, "", "C(",
               "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3".replace("C", "c"), "[nH]1cccc1" * 6 + "cccc"]
    assert len(AROMATIC_64) == len(RING_MAX) == 64 and all(len(s) <= 64 for s in strings)
    want = agree(strings, vocab, 64, what="full width")
    assert want[0]["verdict"] == 0 and want[0]["steps"] == 15 and len(want[0]["wanting"]) == 30
    assert want[1]["formula"][:3] == [130, 0, 64] and want[2]["steps"] == 32 and want[2]["verdict"] == 0
    assert want[3]["verdict"] == 1 and want[3]["atom"] == 0                  # 4 atoms with 30 ring bonds between them
    assert want[4]["formula"][11] == 4 and want[6]["formula"][11] == 64


def test_graph_arrays_that_no_scan_writes(vocab):
    """Counts out of range and a bond end >= natoms give all-zero rows; a bond listed twice counts twice; an entry (a, a) counts
    twice at a and is never an edge; |W| odd; an order outside 1..5 is a sum like any other; a try that is taken back."""
    c, ar, f = K.descriptor("C"), K.descriptor("c"), K.descriptor("F") | 1 << 10
    odd = [(3, [c] * 3, 2, [(0, 3, 1), (1, 2, 1)]), (9, [c] * 8, 0, []), (2, [c] * 2, 9, []), (-1, [], 0, []), (2, [c] * 2, -1, []),
           (0, [], 0, []), (2, [c] * 2, 2, [(0, 1, 1)] * 2), (2, [c] * 2, 1, [(0, 0, 2)]), (2, [c] * 2, 1, [(0, 1, 7)]),
           (2, [c] * 2, 1, [(0, 1, 0)]), (2, [c] * 2, 1, [(0, 1, 65535)]), (2, [ar] * 2, 2, [(0, 1, 5)] * 2),
           (2, [ar] * 2, 2, [(0, 0, 5), (0, 1, 5)]), (3, [ar] * 3, 2, [(0, 1, 5), (2, 1, 5)]), (2, [ar, f], 1, [(0, 1, 5)]),
           (4, [ar] * 4, 3, [(0, 1, 5), (0, 2, 5), (0, 3, 5)]), (8, [ar] * 8, 8, [(i, (i + 1) % 8, 5) for i in range(8)]),
           (1, [ar], 1, [(0, 0, 5)]), (6, [ar] * 6, 7, BACKTRACK), (8, [ar] * 8, 8, [(0, 1, 5)] * 8)]
    natoms = torch.tensor([n for n, _, _, _ in odd], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([nb for _, _, nb, _ in odd], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(odd), 8), 0x7FFFFFFF, dtype=torch.int32, device=DEV)    # (beyond the counts: never read)
    bonds = torch.full((len(odd), 8), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    for r, (_, listed_atoms, _, listed) in enumerate(odd):
        for a, d in enumerate(listed_atoms):
            atoms[r, a] = d
        for e, (a, b, o) in enumerate(listed):
            word = a | b << 8 | o << 16
            bonds[r, e] = word - (1 << 32 if word >> 31 else 0)              # (the uint32 bits in int32 storage)
    want = [H.hydrogens_arrays(n, list(la), nb, list(lb), 8) for n, la, nb, lb in odd]
    agree_arrays(torch.ops.mdt.mol_hydrogens(natoms, atoms, nbonds, bonds, 4096), want)
    assert all(not any(r["hydrogens"] + r["formula"]) and r["verdict"] == 0 for r in want[:6])
    assert want[6]["hydrogens"][:2] == [2, 2] and want[7]["hydrogens"][:2] == [0, 4] and want[10]["hydrogens"][:2] == [0, 0]
    assert want[11]["partner"][:2] == [2, 1] and want[12]["hydrogens"][:2] == [0, 2] and want[13]["verdict"] == 2
    assert (want[14]["verdict"], want[14]["atom"]) == (1, 1) and (want[15]["verdict"], want[15]["steps"]) == (2, 1)
    assert want[18]["steps"] == 4 and want[18]["partner"][:6] == [3, 4, 1, 2, 6, 5]
    want3 = [H.hydrogens_arrays(n, list(la), nb, list(lb), 8, cap=3) for n, la, nb, lb in odd]
    assert want3[18]["verdict"] == 3 and want3[16]["verdict"] == 3
    agree_arrays(torch.ops.mdt.mol_hydrogens(natoms, atoms, nbonds, bonds, 3), want3)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_max_steps_is_honoured(cap, vocab):
    strings = ["c1ccc2ccccc2c1", "c1ccc2cccc2cc1", "c1ccccc1", "cc", "c1cccc1", "CCO", "", "o1(C)cccc1", AROMATIC_64]
    want = agree(strings, vocab, 64, cap=cap, what=cap)
    assert [r["verdict"] for r in want[:2]] == [3, 3] and want[2]["verdict"] == (0 if cap == 3 else 3)
    assert [r["verdict"] for r in want[3:]] == [0, 2, 0, 0, 1, 3]            # decided rows are never wrong, whatever the cap


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry point on outputs pre-filled with 0xA5 bytes: every word comes out defined, zero beyond the counts."""
    strings = pool[::3] + ["", "C(", AROMATIC_64]
    for L in (64, 37):
        rows = [s[:L] for s in strings]
        natoms, atoms, nbonds, bonds = graph_arrays(rows, vocab, L)
        R = len(rows)
        poison = lambda *shape, dtype: torch.full(shape, 0xA5 if dtype == torch.uint8 else -0x5A5A5A5B, dtype=dtype, device=DEV)  # noqa: E731
        out = (poison(R, L, dtype=torch.uint8), poison(R, L, dtype=torch.uint8), poison(R, dtype=torch.uint8), poison(R, dtype=torch.int32),
               poison(R, 13, dtype=torch.int32))
        guard = [poison(64, dtype=t.dtype) for t in out]                      # (allocated next to the outputs; must come back as filled)
        with torch.cuda.device(DEV):
            rt.check(rt.load_library().mdt_mol_hydrogens(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, 4096,
                                                         *[rt.ptr(t) for t in out], rt.current_stream()))
        want = [H.string_hydrogens(s, H.MAX_STEPS, L) for s in rows]
        agree_arrays(out, want, what=L)
        n = natoms.long().unsqueeze(1)
        beyond = torch.arange(L, device=DEV).unsqueeze(0) >= n
        assert not out[0][beyond].any() and not out[1][beyond].any()
        assert all(torch.equal(g, poison(64, dtype=g.dtype)) for g in guard)


def test_the_same_call_twice_gives_identical_bits(pool, vocab):
    graph = graph_arrays(pool, vocab, 64)
    first = torch.ops.mdt.mol_hydrogens(*graph, 4096)
    second = torch.ops.mdt.mol_hydrogens(*graph, 4096)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_screening_with_kekulize_end_to_end():
    """Three targets, six candidates each on the small model of the graph-identity test.  c1cccc1 is never kept and carries bit 64
    under kekulize=True; benzene in either spelling stays eligible; kekulize=False returns what the call returns without it."""
    G2, N2, K2, L2, T = 3, 6, 3, 32, 4
    vocab = SmilesVocabulary([None] + list("CNOcno1()-=#[H]"))
    order = [["c1cccc1", "c1ccccc1", "C1=CC=CC=C1", "CCO", "n1cccc1", "c1cc[nH]c1"],
             ["c1ccccc1", "c1cccc1", "C(", "o1(C)cccc1", "c1ccoc1", "C1=CC=CC=C1"],
             ["CC", "c", "cC", "cc", "c1ccnc1", "c1ccncc1"]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]            # row c * G + g
    tokens = vocab.encode(strings, L2)
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, vocabulary=vocab)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, kekulize=True, forward_noise=noise(), **kw)
    again = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, kekulize=True, forward_noise=noise(), **kw)
    plain = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, forward_noise=noise(), **kw)
    off = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, kekulize=False, forward_noise=noise(), **kw)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # False: today's result, field for field; and repeatable
        for a, b in ((getattr(off, name), getattr(plain, name)), (getattr(again, name), getattr(out, name))):
            assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    flagged = np.array([64 if H.string_hydrogens(s)["verdict"] else 0 for s in strings], dtype=np.uint8).reshape(N2, G2)
    assert flagged[:, 0].tolist() == [64, 0, 0, 0, 64, 0] and flagged[:, 1].tolist() == [0, 64, 0, 64, 0, 0]
    assert flagged[:, 2].tolist() == [0, 64, 64, 0, 64, 0]
    assert not (plain.status.cpu().numpy()[flagged != 0] & 96).any()         # smiles_check alone lets every one of them pass
    want = plain.status.cpu().numpy() | flagged
    assert out.status.dtype == torch.uint8 and np.array_equal(out.status.cpu().numpy(), want)
    index = [[c for c in plain.index[g].tolist() if c >= 0 and not flagged[c, g]][:K2] for g in range(G2)]
    assert out.index.tolist() == [kept + [-1] * (K2 - len(kept)) for kept in index] and out.count.tolist() == [len(k) for k in index]
    assert all(0 not in kept for kept in index[:1]) and out.status[0, 0] & 64 and not out.status[1, 0] & 64 and not out.status[2, 0] & 64
    assert all(want[c, g] & 64 == 0 for g in range(G2) for c in index[g])    # kept rows never carry the bit
