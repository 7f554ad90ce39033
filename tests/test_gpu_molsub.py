"""-m gpu: mdt_sub_match (csrc/k_molsub.hip), has_substructure(), SubstructureSet and the screening call with ``require`` /
``forbid`` on the device.  Every comparison is exact: every match and undecided word and every flag against the plain-int reference
tests/molsub_ref.py (whose graphs are tests/molkey_ref.py's).  No row here can run longer than its step cap: at most 64 roots of
4096 steps per (row, pattern)."""
import functools

import numpy as np
import pytest
import torch

import molkey_ref as K
import molsub_ref as B
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, SubstructureSet, has_substructure,
                                              screen_tokens_diverse)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

RING_SYSTEM = "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3"              # (as the graph key's full-width test)
RING_MAX = "*" + "0123456789" + ("*" + "0123456789" * 2) * 2 + "*" + "0123456789"     # 64 tokens, 4 atoms, 30 ring bonds
CAP_PATTERN, CAP_UNDECIDED, CAP_MATCH = "C.C.C.C.C.C.CN", "C" * 62 + ".N", "C" * 61 + "CN"
ROWS_PER_BLOCK = 4                                                          # k_sub_match: waves (rows in flight) of a workgroup


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def vocab(spelled):
    chars = set(S.CHARS) | set("".join(s for _, sp in spelled for s in sp)) | set("$:*%\\/")
    return SmilesVocabulary([None] + sorted(chars))


@pytest.fixture(scope="module")
def pool(spelled):
    """Strings of at most 64 tokens: spellings, and mutated rows of which most are no molecule."""
    rng = np.random.default_rng(5)
    broken = [s[:int(rng.integers(1, len(s) + 1))] + ("(" if r % 3 else "") for r, s in enumerate(S.mutated_rows(256)) if s]
    assert sum(not B.graph_of(s)[0] for s in broken) > 0.5 * len(broken)
    return [s for _, sp in spelled[:60] for s in sp] + broken


@functools.lru_cache(maxsize=None)
def verdict(pattern, target):
    return B.string_match(pattern, target)[0]


def want_words(targets, patterns):
    rows = [[verdict(p, t) for p in patterns] for t in targets]
    return ([sum(1 << q for q, v in enumerate(row) if v == B.MATCH) for row in rows],
            [sum(1 << q for q, v in enumerate(row) if v == B.UNDECIDED) for row in rows])


def graph_arrays(strings, vocabulary, width):
    """The graph arrays of mdt::mol_graph, int32 on the device; a string that is no molecule has no atoms."""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    return torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]


def bits(word):
    return word.cpu().numpy().view(np.uint32).tolist()


def agree(targets, patterns, vocabulary, L, LP, need=0, ban=0, what=None):
    match, undecided, flags = torch.ops.mdt.sub_match(*graph_arrays(targets, vocabulary, L), *graph_arrays(patterns, vocabulary, LP),
                                                      need, ban)
    torch.cuda.synchronize()
    assert match.dtype == undecided.dtype == torch.int32 and flags.dtype == torch.uint8 and match.shape == flags.shape == (len(targets),)
    want_m, want_u = want_words(targets, patterns)
    got_m, got_u = bits(match), bits(undecided)
    for r, t in enumerate(targets):
        assert (got_m[r], got_u[r]) == (want_m[r], want_u[r]), (what, r, t, patterns)
    assert flags.tolist() == [B.flag(m, u, need, ban) for m, u in zip(want_m, want_u)], what
    return want_m, want_u


def patterns_of(P, LP, seed):
    rng = np.random.default_rng(seed)
    source = B.PATTERNS + B.EVERYDAY + ["CC(C)C", "OCC", "C1CC1C", "*C", "C(C1)1", "[nH]", "Cl", "C(", ""]
    return [source[int(rng.integers(len(source)))][:LP] for _ in range(P)]   # (cut short: some are no molecule, which is a case)


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 257])
@pytest.mark.parametrize("L", [1, 33, 64])
def test_sub_match_row_shapes(L, R_, pool, vocab):
    rng = np.random.default_rng(100 * L + R_)
    targets = [pool[int(rng.integers(len(pool)))][:L] for _ in range(R_)]
    P, LP = [(1, 17), (31, 32), (32, 1), (32, 32), (31, 17)][(L + R_) % 5]
    patterns = patterns_of(P, LP, R_)
    need = 1 << int(rng.integers(P))
    ban = ((1 << P) - 1) & ~need & int(rng.integers(1 << 32))
    agree(targets, patterns, vocab, L, LP, need, ban, what=(L, R_, P, LP))


@pytest.mark.parametrize("P", [1, 31, 32])
@pytest.mark.parametrize("LP", [1, 17, 32])
def test_sub_match_pattern_shapes(LP, P, pool, vocab):
    targets = pool[:40:3] + pool[-6:]
    want_m, _ = agree(targets, patterns_of(P, LP, 7 * P + LP), vocab, 64, LP, what=(P, LP))
    assert P == 1 or (any(want_m) and not all(want_m))


def test_full_width_rows_and_patterns(vocab):
    targets = ["C" * 64, RING_MAX, RING_SYSTEM, "C1" * 32, "c1ccccc1" * 8, "*" * 64, "", "C(", CAP_UNDECIDED, CAP_MATCH]
    patterns = ["C" * 32, "*" * 32, "c1ccccc1c1ccccc1", "C1CCCCCCCCCCCCCCC1", "C(C)(C)C", "*.*.*.*", CAP_PATTERN, "C", "cc"]
    assert len(RING_MAX) == 64 and all(len(t) <= 64 for t in targets) and all(len(p) <= 32 for p in patterns)
    want_m, want_u = want_words(targets, patterns)
    assert want_u[8] == 1 << 6 and want_m[9] >> 6 & 1 and not any(want_u[:8])                   # the two cap rows: undecided, match
    assert want_m[0] == 0b010100001 | 1 << 1 and want_m[6] == want_m[7] == 0                    # the chain; the rows that are no molecule
    match, undecided, status, position = has_substructure(vocab.encode(targets, 64), SubstructureSet(patterns, vocab), vocab, DEV)
    torch.cuda.synchronize()
    assert match.dtype == undecided.dtype == torch.bool and match.shape == undecided.shape == (len(targets), len(patterns))
    for r, t in enumerate(targets):
        for q, p in enumerate(patterns):
            assert (bool(match[r, q]), bool(undecided[r, q])) == (bool(want_m[r] >> q & 1), bool(want_u[r] >> q & 1)), (t, p)
    assert not (match & undecided).any()
    assert status.tolist() == [S.check(t)[0] for t in targets] and status.tolist()[7] == 32 and position.tolist()[7] == 2


def test_the_highest_root_and_a_match_behind_a_dead_end(vocab):
    # only root 63 can start: the pattern's first atom is the row's last
    _, roots = B.match_arrays(64, B.graph_of("C" * 63 + "N")[0], 63, B.graph_of("C" * 63 + "N")[1], 2, *[x for g in [B.graph_of("NC")]
                                                                                                      for x in (g[0], 1, g[1])])
    assert [(r, v) for r, v, _ in roots] == [(63, B.MATCH)]
    # root 0 walks into two methyl groups before it finds the arm that carries the oxygen
    branched = B.graph_of("C(C)(C)CO")
    _, roots = B.match_arrays(5, branched[0], 4, branched[1], 3, B.graph_of("CCO")[0], 2, B.graph_of("CCO")[1])
    assert (0, B.MATCH, 4) in roots and 4 > 3 - 1                            # more steps than atoms to place: it went back
    targets = ["C" * 63 + "N", "N" + "C" * 63, "C" * 64, "C(C)(C)CO", "C(C)(C)CC", "OCC(C)(C)C(C)(C)C(C)(C)C"]
    want_m, want_u = agree(targets, ["NC", "CCO", "N", "C(C)(C)(C)CCO", "OCC(C)(C)C(C)(C)C(C)C"], vocab, 64, 32, what="roots")
    assert want_m == [0b00101, 0b00101, 0, 0b00010, 0, 0b11010] and not any(want_u)


def test_graph_arrays_that_no_scan_writes(vocab):
    """Counts outside [0, width], a bond that names a missing atom, an order outside 1..5, on either side: no match, decided.  A
    bond listed twice asks the same thing twice; a bond of an atom to itself is part of what the atom accepts."""
    c = K.descriptor("C")
    odd = [(3, 2, [(0, 3, 1), (1, 2, 1)]), (9, 0, []), (2, 9, []), (-1, 0, []), (2, -1, []), (2, 2, [(0, 1, 1)] * 2), (2, 1, [(0, 0, 2)]),
           (2, 1, [(0, 1, 7)]), (2, 2, [(1, 1, 2), (1, 0, 1)]), (3, 2, [(0, 1, 1), (2, 1, 1)]), (1, 0, []), (4, 3, [(0, 1, 1), (0, 2, 1), (0, 3, 1)])]
    natoms = torch.tensor([n for n, _, _ in odd], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([nb for _, nb, _ in odd], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(odd), 8), c, dtype=torch.int32, device=DEV)
    bonds = torch.zeros(len(odd), 8, dtype=torch.int32, device=DEV)
    for r, (_, _, listed) in enumerate(odd):
        for e, (a, b, o) in enumerate(listed):
            bonds[r, e] = a | b << 8 | o << 16
    match, undecided, _ = torch.ops.mdt.sub_match(natoms, atoms, nbonds, bonds, natoms, atoms, nbonds, bonds, 0, 0)
    torch.cuda.synchronize()
    want = [sum(1 << q for q, (m, mb, pb) in enumerate(odd) if B.match_arrays(n, [c] * 8, nb, tb, m, [c] * 8, mb, pb, 8, 8)[0] == B.MATCH)
            for n, nb, tb in odd]
    assert bits(match) == want and not undecided.any()
    assert [w for w in want[:5]] == [0] * 5 and all(not w >> q & 1 for w in want for q in (0, 1, 2, 3, 4, 7))
    assert want[5] >> 5 & 1 and want[8] >> 8 & 1 and want[8] >> 6 & 1 and not want[5] >> 6 & 1 and want[11] >> 9 & 1 and want[7] == 1 << 10


def test_flags_for_every_role_of_a_matched_a_missing_and_an_undecided_pattern(vocab):
    targets, patterns = [CAP_UNDECIDED, "CCO"], ["C", "S", CAP_PATTERN]      # row 0: match, none, undecided; row 1: match, none, none
    graphs = graph_arrays(targets, vocab, 64) + graph_arrays(patterns, vocab, 32)
    assert want_words(targets, patterns) == ([1, 1], [4, 0])
    seen = set()
    for roles in np.ndindex(3, 3, 3):                                        # per pattern: neither, need, ban
        need = sum(1 << q for q, role in enumerate(roles) if role == 1)
        ban = sum(1 << q for q, role in enumerate(roles) if role == 2)
        match, undecided, flags = torch.ops.mdt.sub_match(*graphs, need, ban)
        assert (bits(match), bits(undecided)) == ([1, 1], [4, 0])
        assert flags.tolist() == [B.flag(1, 4, need, ban), B.flag(1, 0, need, ban)], roles
        seen.add(tuple(flags.tolist()))
    assert seen == {(0, 0), (128, 0), (128, 128)}
    # all 32 bits: pattern 31 is the sign bit of the int32 word
    patterns = ["S"] * 31 + ["O"]
    match, undecided, flags = torch.ops.mdt.sub_match(*graph_arrays(targets, vocab, 64), *graph_arrays(patterns, vocab, 32), 1 << 31, 1)
    assert bits(match) == [0, 1 << 31] and flags.tolist() == [128, 0]


def test_has_substructure_end_to_end(spelled, vocab):
    fragments = SubstructureSet(B.EVERYDAY, vocab)
    strings = [s for _, sp in spelled[:50] for s in sp] + ["", "C(", "CC(=O)O", "N#CC#N", "FC(F)(F)c1ccccc1", "C1=CC=CC=C1"]
    ids = vocab.encode(strings, 64)
    spread = torch.zeros(len(strings), 64, dtype=torch.int16)                # zeros anywhere: a molecule is its compacted row
    spread[:, ::2] = ids[:, :32].to(torch.int16)
    fits = [r for r, s in enumerate(strings) if len(s) <= 32]
    want_m, want_u = want_words(strings, B.EVERYDAY)
    for tok, rows in ((spread, fits), (ids, range(len(strings)))):
        match, undecided, status, position = has_substructure(tok, fragments, vocab, DEV)
        for r in rows:
            assert [int(x) for x in match[r]] == [want_m[r] >> q & 1 for q in range(8)], strings[r]
        assert not undecided.any() and not any(want_u)
    for g, sp in spelled[:50]:                                               # a decided answer does not depend on the spelling
        assert len({want_m[strings.index(s)] for s in sp}) == 1
    assert fragments.on(DEV) is fragments.on(DEV) and fragments.on(DEV)[1].shape == (8, 8)
    as_list = has_substructure(ids, list(B.EVERYDAY), vocab, DEV)
    assert torch.equal(as_list[0], match) and torch.equal(as_list[1], undecided)
    by = dict(zip(strings, want_m))
    assert by["CC(=O)O"] == 0b00010001 and by["N#CC#N"] == 0b00100010 and by["FC(F)(F)c1ccccc1"] == 0b10000100 and by["C1=CC=CC=C1"] == 0
    with pytest.raises(ValueError, match=r"pattern 1 'C\(\(' does not pass smiles_check\(\): malformed at position 2"):
        SubstructureSet(["C", "C(("], vocab).on(DEV)
    with pytest.raises(ValueError, match="pattern 0 'C=C=C=O=C' .* overvalent at position 6"):
        has_substructure(ids, ["C=C=C=O=C"], vocab, DEV)


def test_screening_with_require_and_forbid_end_to_end():
    """Four targets, eight candidates each on the small model of the graph-identity test: a kept candidate must contain C=O and may
    not contain C#N.  Bit 128 sits where the reference says, kept rows never carry it, and they are the best of the rest."""
    G2, N2, K2, L2, T = 4, 8, 3, 32, 4
    vocab = SmilesVocabulary([None] + list("CNO1()-=#"))
    order = [["CC=O", "CCO", "O=CC#N", "C(", "OC(C)=O", "N#CC", "C1CC1C=O", "CC(=O)N"],
             ["N#CC=O", "O=C", "CCN", "C(=O)C", "C(", "O=CCC#N", "CC", "NC=O"],
             ["CCC", "CCO", "C#N", "CN", "C1CC1", "C(", "OCC", "C=C"],
             ["O=CO", "C(C)=O", "CC(C)=O", "O=C1CC1", "NC(N)=O", "O=CC=O", "OC=O", "CC=O"]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]            # row c * G + g
    tokens = vocab.encode(strings, L2)
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, vocabulary=vocab)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, require=["C=O"], forbid=["C#N"], forward_noise=noise(), **kw)
    plain = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, forward_noise=noise(), **kw)
    none = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, require=None, forbid=None, forward_noise=noise(), **kw)
    sets = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, require=SubstructureSet(["C=O"], vocab),
                                 forbid=SubstructureSet(["C#N"], vocab), forward_noise=noise(), **kw)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # both at None: today's result, field for field
        for a, b in ((getattr(none, name), getattr(plain, name)), (getattr(sets, name), getattr(out, name))):
            assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    want_m, want_u = want_words(strings, ["C=O", "C#N"])
    flagged = np.array([B.flag(m, u, 1, 2) for m, u in zip(want_m, want_u)], dtype=np.uint8).reshape(N2, G2)
    assert flagged[:, 2].all() and flagged.sum() // 128 == 4 + 5 + 8 and not flagged[:, 3].any()
    want = plain.status.cpu().numpy() | flagged
    assert out.status.dtype == torch.uint8 and np.array_equal(out.status.cpu().numpy(), want)
    index = [[c for c in plain.index[g].tolist() if c >= 0 and not flagged[c, g]][:K2] for g in range(G2)]
    count = [len(kept) for kept in index]
    assert out.index.tolist() == [kept + [-1] * (K2 - len(kept)) for kept in index] and out.count.tolist() == count == [3, 3, 0, 3]
    assert all(want[c, g] & 128 == 0 for g in range(G2) for c in index[g])   # kept rows never carry the bit
    assert float(((out.status & 128) == 0).float().mean()) == 1 - 17 / 32
