"""-m gpu: mdt_mol_graph, mdt_mol_key and mdt_key_flags (csrc/k_molgraph.hip), KnownSet.mol_keys and the screening calls with
``identity="graph"`` on the device.  Every comparison is exact: atoms, bonds, status, position and keys against the string-level
reference tests/molkey_ref.py (whose status and position are tests/smiles_ref.py's), the flags against a numpy loop."""
import numpy as np
import pytest
import torch

import molkey_ref as K
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, SmilesVocabulary, mol_graph, mol_key, screen_tokens_diverse,
                                              smiles_check)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

EQUAL, DIFFERENT = K.EQUAL_PAIRS, K.DIFFERENT_PAIRS

RING_MAX = "*" + "0123456789" + ("*" + "0123456789" * 2) * 2 + "*" + "0123456789"     # 64 tokens, 4 atoms, 30 ring bonds


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def vocab(spelled):
    """One id per character of every row the tests write."""
    chars = set(S.CHARS) | set("".join(s for _, sp in spelled for s in sp)) | set("$:*%\\/")
    return SmilesVocabulary([None] + sorted(chars))


def on_device(ids, vocabulary):
    """mol_graph() and mol_key() as numpy: (natoms, atoms, nbonds, bonds, status, position, key uint64)."""
    graph = mol_graph(ids, vocabulary, DEV)
    key, status, position = mol_key(ids, vocabulary, DEV)
    torch.cuda.synchronize()
    R, L = ids.shape
    assert [tuple(t.shape) for t in graph] == [(R,), (R, L), (R,), (R, L), (R,), (R,)] and all(t.dtype == torch.int64 for t in graph)
    assert key.dtype == torch.int64 and key.shape == (R,)
    assert torch.equal(status, graph[4]) and torch.equal(position, graph[5])
    return tuple(t.cpu().numpy() for t in graph) + (key.cpu().numpy().view(np.uint64),)


def agree(strings, vocabulary, L, ids=None, what=None):
    """Every output of the device against the reference, row by row, bit for bit."""
    ids = vocabulary.encode(strings, L) if ids is None else ids
    natoms, atoms, nbonds, bonds, status, position, key = on_device(ids, vocabulary)
    for r, s in enumerate(strings):
        st, pos, want_atoms, want_bonds = K.graph(s)
        words = [a | b << 8 | o << 16 for a, b, o in want_bonds]
        got = (int(status[r]), int(position[r]), int(natoms[r]), atoms[r].tolist(), int(nbonds[r]), bonds[r].tolist(), int(key[r]))
        want = (st, pos, len(want_atoms), want_atoms + [0] * (ids.shape[1] - len(want_atoms)), len(words),
                words + [0] * (ids.shape[1] - len(words)), K.string_key(s))
        assert got == want, (what, r, s, got, want)
    return key


def test_the_agreed_pairs_and_the_three_tables(vocab):
    strings = [s for pair in EQUAL + DIFFERENT for s in pair] + [s for s, _, _ in S.TABLES] + [""]
    key = agree(strings, vocab, 32)
    by = dict(zip(strings, key.tolist()))
    for a, b in EQUAL:
        assert by[a] == by[b] != 0, (a, b)
    for a, b in DIFFERENT:
        assert by[a] != by[b] and by[a] and by[b], (a, b)
    assert all(by[s] != 0 for s in S.OK_TABLE) and by[""] == 0
    assert all(by[s] == 0 for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE)


def test_random_spellings(spelled, vocab):
    strings = [s for _, sp in spelled for s in sp]
    for s in strings:
        assert S.check(s) == (S.OK, -1)                                      # (a row that is no molecule would pass on key 0)
    key = agree(strings, vocab, 64).reshape(len(spelled), -1)
    assert (key != 0).all() and (key == key[:, :1]).all()                    # one key per graph, whatever the spelling
    assert len(set(key[:, 0].tolist())) >= len({tuple(sorted(g.descriptors())) for g, _ in spelled})


def test_mutated_rows(vocab):
    rows = S.mutated_rows()
    ids = vocab.encode(rows, 32)
    key = agree(rows, vocab, 32, ids=ids)
    status, position = smiles_check(ids, vocab, DEV)
    want = [S.check(r) for r in rows]
    assert status.tolist() == [w[0] for w in want] and position.tolist() == [w[1] for w in want]
    for v in (S.OK, S.MALFORMED, S.OVERVALENT):                              # every verdict occurs
        assert sum(w[0] == v for w in want) >= 0.05 * len(rows), v
    assert ((key == 0) == np.array([w[0] != 0 or r == "" for w, r in zip(want, rows)])).all()    # key 0 exactly where no molecule
    again = on_device(ids, vocab)                                            # two calls give equal results
    first = on_device(ids, vocab)
    assert all(np.array_equal(a, b) for a, b in zip(again, first)) and np.array_equal(first[6], key)


@pytest.mark.parametrize("R_", [1, 63, 64, 65])                            # one workgroup of mdt_mol_graph takes 64 rows
@pytest.mark.parametrize("L", [1, 32, 33, 64])                             # the limits, and a width that is no multiple of four
def test_shapes(L, R_, spelled, vocab):
    rng = np.random.default_rng(100 * L + R_)
    pool = [s for _, sp in spelled for s in sp] + S.mutated_rows(512)
    strings = [pool[int(rng.integers(len(pool)))][:L] for _ in range(R_)]
    agree(strings, vocab, L, what=(L, R_))


def test_full_width_rows(vocab):
    chain = "C" * 64                                                         # 64 atoms, 63 bonds: every lane a root
    strings = [chain, RING_MAX, "C1" * 32, "C%12" * 16, "C(" * 21 + "C" + ")" * 21, "[13CH4]" * 9, "c1ccccc1" * 8,
               "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3", "[4095C]", "[2049C-9]", "*", "C" * 63 + "(", "C" * 63 + "N"]
    assert len(RING_MAX) == 64 and S.check(RING_MAX) == (S.OK, -1) and len(K.graph(RING_MAX)[3]) == 33
    assert [len(x) for x in K.graph(chain)[2:]] == [64, 63] and S.check("C1" * 32) == (S.OK, -1)
    key = agree(strings, vocab, 64)
    assert key[0] != 0 and key[0] != key[-1] and key[-2] == 0
    natoms, _, nbonds, _, _, _, _ = on_device(vocab.encode([chain, RING_MAX], 64), vocab)
    assert natoms.tolist() == [64, 4] and nbonds.tolist() == [63, 33]


def test_mol_key_of_graph_arrays_no_scan_writes():
    """Counts outside [1, L] x [0, L] and a bond that names an atom the row does not have -> key 0 (nothing beyond the counts is
    read); a bond listed twice and a bond of an atom to itself count at both ends, as tests/molkey_ref.py's key counts them."""
    c = K.descriptor("C")
    natoms = torch.tensor([3, 9, 2, -1, 2, 2, 2], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([2, 0, 9, 0, -1, 2, 1], dtype=torch.int32, device=DEV)
    atoms = torch.full((7, 8), c, dtype=torch.int32, device=DEV)
    bonds = torch.zeros(7, 8, dtype=torch.int32, device=DEV)
    bonds[0, :2] = torch.tensor([0 | 3 << 8 | 1 << 16, 1 | 2 << 8 | 1 << 16])
    bonds[5, :2] = 0 | 1 << 8 | 1 << 16
    bonds[6, 0] = 0 | 0 << 8 | 2 << 16
    key = torch.ops.mdt.mol_key(natoms, atoms, nbonds, bonds)
    torch.cuda.synchronize()
    want = [0] * 5 + [K.key([c, c], [(0, 1, 1)] * 2), K.key([c, c], [(0, 0, 2)])]
    assert want[5] and want[6] and want[5] != want[6]
    assert key.dtype == torch.int64 and key.cpu().numpy().view(np.uint64).tolist() == want
    # full width: 64 atoms are a graph of L = 64, a bond end of 64 is not
    wide = torch.zeros(1, 64, dtype=torch.int32, device=DEV)
    wide[0, 0] = 0 | 64 << 8 | 1 << 16
    key = torch.ops.mdt.mol_key(torch.tensor([64], dtype=torch.int32, device=DEV), torch.full((1, 64), c, dtype=torch.int32, device=DEV),
                                torch.tensor([1], dtype=torch.int32, device=DEV), wide)
    torch.cuda.synchronize()
    assert key.tolist() == [0]


def test_zeros_scattered_through_a_row(vocab):
    rng = np.random.default_rng(7)
    strings = [s for s, _, _ in S.TABLES] + [s for pair in EQUAL for s in pair]
    ids = vocab.encode(strings, 32).numpy()
    spread = np.zeros((len(strings), 64), np.int64)
    for r, s in enumerate(strings):                                          # the same tokens at random places, in order
        spread[r, np.sort(rng.choice(64, len(s), replace=False))] = ids[r, :len(s)]
    for dtype in (torch.int64, torch.int16):
        agree(strings, vocab, 64, ids=torch.from_numpy(spread).to(dtype), what=dtype)


# ----------------------------------------------------------------------------------------------------------------------
# the flags
# ----------------------------------------------------------------------------------------------------------------------
def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def ref_flags(key, N, G, known):
    flags = np.zeros(N * G, np.uint8)
    known = set(int(k) for k in known)
    for g in range(G):
        seen = set()
        for c in range(N):
            k = int(key[c * G + g])
            if k:
                flags[c * G + g] = (4 if k in seen else 0) | (8 if k in known else 0)
                seen.add(k)
    return flags


@pytest.mark.parametrize("N", [1, 2, 1024])
def test_key_flags(N):
    G = 3
    rng = np.random.default_rng(N)
    pool = np.array([0, 1, 2, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 5, 2 ** 64 - 1, 77, 1 << 40], dtype=np.uint64)      # both halves of uint64
    key = pool[rng.integers(len(pool), size=N * G)]
    key[0 * G + 1] = 0                                                       # group 1: the first occurrence has key 0 ...
    if N > 1:
        key[1 * G + 1] = 0                                                   # ... twice: no duplicate of "no molecule"
    key[2::G] = 77                                                           # group 2: all keys equal
    known = np.array([1, 77, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)         # ascending as unsigned; hits at both ends
    for kn in (known, known[:1], known[-1:], known[:0]):
        got = torch.ops.mdt.key_flags(dev64(key), N, dev64(kn) if len(kn) else None)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref_flags(key, N, G, kn)), (N, kn)
    empty = torch.ops.mdt.key_flags(dev64(key), N, dev64(known[:0]))         # M = 0 as an empty tensor
    assert np.array_equal(empty.cpu().numpy(), ref_flags(key, N, G, []))
    want = ref_flags(key, N, G, known).reshape(N, G)
    assert want[0, 1] == 0 and want[0, 2] == 8 and (N == 1 or (want[1, 1] == 0 and (want[1:, 2] == 12).all()))


# ----------------------------------------------------------------------------------------------------------------------
# the known set and the screening call
# ----------------------------------------------------------------------------------------------------------------------
def test_known_set_keys_on_respelled_rows(spelled, vocab):
    picked = [sp for g, sp in spelled[:60] if len(g.atoms) > 2 and max(len(s) for s in sp) <= 32]
    rows = [s for sp in picked for s in sp] + ["C(", "CF(C)", "C"]
    known = KnownSet(vocab.encode(rows, 32), 32)
    keys = known.mol_keys(vocab, DEV)
    torch.cuda.synchronize()
    want = sorted({K.string_key(s) for s in rows} - {0})
    assert len(want) == len({K.string_key(sp[0]) for sp in picked}) + 1 < len(known)      # respellings count once, non-molecules drop out
    assert keys.dtype == torch.int64 and keys.cpu().numpy().view(np.uint64).tolist() == want
    assert any(k >= 2 ** 63 for k in want) and any(k < 2 ** 63 for k in want)             # the order is the unsigned one
    assert known.mol_keys(vocab, DEV) is keys


def test_screening_by_graph_identity_end_to_end():
    """Two targets, eight candidates each: respellings of ethanol and of methylcyclopropane, one row that is no molecule.  The known
    set spells ethanol a fourth way, so by string nothing is known and nothing repeats; by graph every ethanol is known and only
    the lowest-c methylcyclopropane of a target is kept."""
    G2, N2, K2, L2, T = 2, 8, 2, 32, 4
    vocab = SmilesVocabulary([None] + list("CO1()-"))                        # (ids below 64: the distance filter takes them)
    ethanol, mcp = ["CCO", "OCC", "C(O)C", "C-C-O"], ["C1CC1C", "CC1CC1", "C1(C)CC1"]
    order = [[ethanol[0], mcp[0], ethanol[1], "C(", mcp[1], ethanol[2], mcp[2], ethanol[3]],
             [mcp[1], mcp[2], ethanol[3], ethanol[2], "C(", mcp[0], ethanol[0], ethanol[1]]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]                          # row c * G + g
    tokens = vocab.encode(strings, L2)
    known = KnownSet(vocab.encode(["C(C)O", "CCCC"], L2), L2)
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, known_tokens=known, vocabulary=vocab)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, identity="graph", forward_noise=noise(), **kw)
    plain = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, forward_noise=noise(), **kw)
    string = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, identity="string", forward_noise=noise(), **kw)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # "string" is today's result, field for field
        a, b = getattr(string, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert plain.status.cpu().numpy().reshape(-1).tolist() == [32 if s == "C(" else 0 for s in strings]       # by string: all distinct, all novel
    keys = np.array([K.string_key(s) for s in strings], dtype=np.uint64)
    want = ref_flags(keys, N2, G2, [K.string_key("C(C)O"), K.string_key("CCCC")]) | plain.status.cpu().numpy().reshape(-1)
    status = out.status.cpu().numpy()
    assert status.dtype == np.uint8 and np.array_equal(status.reshape(-1), want)
    assert status[:, 0].tolist() == [8, 0, 12, 32, 4, 12, 4, 12] and status[:, 1].tolist() == [0, 4, 8, 12, 32, 4, 12, 12]
    assert out.count.tolist() == [1, 1] and out.index.tolist() == [[1, -1], [0, -1]]       # the lowest-c spellings
    assert torch.equal(out.tokens[:, 0].cpu(), tokens[[1 * G2 + 0, 0 * G2 + 1]]) and not out.tokens[:, 1].any()
    assert float(((out.status & 8) == 0).float().mean()) == 0.5 and float(((plain.status & 8) == 0).float().mean()) == 1.0
    # min_distance stays a filter on the strings of eligible candidates: graph identity left one per target, so it changes nothing
    far = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, identity="graph", min_distance=3, forward_noise=noise(), **kw)
    assert torch.equal(far.index, out.index) and torch.equal(far.status, out.status)
