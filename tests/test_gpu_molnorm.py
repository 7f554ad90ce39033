"""-m gpu: mdt_mol_normalize (csrc/k_molnorm.hip), mol_normalize(), the ``normalize=`` keyword of the key, fingerprint and similarity
calls, has_substructure_normalized() and the screening call with ``normalize`` on the device.  Every comparison is exact: the atom
words, the bond words and the flags against the plain-int reference tests/molnorm_ref.py (whose graphs are tests/molkey_ref.py's,
whose hydrogens and Kekule structure are tests/molh_ref.py's and whose ring sizes are tests/molring_ref.py's).  No row here can run
long: at most nbonds searches of at most natoms levels a row."""
import numpy as np
import pytest
import torch

import molfp_ref as F
import molh_ref as H
import molkey_ref as K
import molnorm_ref as N
import molsub_ref as B
import poison_util as P
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, SmilesVocabulary, has_substructure, has_substructure_normalized,
                                              mol_fingerprint, mol_key, mol_normalize, nearest_known_tanimoto, runtime as rt,
                                              screen_tokens_diverse, tanimoto)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 4                                                          # k_mol_normalize: waves (rows) of a workgroup
NO_MOLECULE = ["", "C(", "C1CC", "C=C=C=O=C", "c1ccccc", "Xx"]
NO_KEKULE = ["c1cccc1", "n1cccc1", "c1ccccc1c", "cF"]                         # verdict != 0: they come back as written
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def pool(spelled):
    """Strings of at most 64 tokens: the table, the pairs, the 2,000 random spellings, rows that pass through, mutated rows."""
    rows = list(N.TABLE) + [s for pair in N.PAIRS for s in pair] + [s for _, sp in spelled for s in sp] + NO_MOLECULE + NO_KEKULE
    rows += [s[:64] for s in S.mutated_rows(128)]
    assert all(len(s) <= 64 for s in rows) and sum(N.string_normal(s)["flags"] >> 1 & 1 for s in rows) > 500
    return rows


@pytest.fixture(scope="module")
def vocab(pool):
    return SmilesVocabulary([None] + sorted(set(S.CHARS) | set("".join(pool)) | set("$:*%\\/csnopbBPSI")))


def op_inputs(strings, vocabulary, width):
    """-> the eight inputs of mdt::mol_normalize on the device, by the four launches that come before it"""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]
    hydrogens, partner, verdict, _, _ = torch.ops.mdt.mol_hydrogens(*graph, H.MAX_STEPS)
    bond_ring = torch.ops.mdt.mol_rings(*graph, hydrogens, None, None)[0]
    return (*graph, hydrogens, partner, verdict, bond_ring)


def agree_arrays(got, want, what=None):
    """got: the three tensors of the op; want: the reference's rows."""
    torch.cuda.synchronize()
    atoms, bonds, flags = got
    assert (atoms.dtype, bonds.dtype, flags.dtype) == (torch.int32, torch.int32, torch.uint8)
    assert (atoms.long() & MASK32).tolist() == [r["atoms"] for r in want], what
    assert (bonds.long() & MASK32).tolist() == [r["bonds"] for r in want], what
    assert flags.tolist() == [r["flags"] for r in want], what


def agree(strings, vocabulary, L, what=None):
    want = [N.string_normal(s, L) for s in strings]
    agree_arrays(torch.ops.mdt.mol_normalize(*op_inputs(strings, vocabulary, L)), want, what)
    return want


def unsigned(t):
    return [int(k) & MASK64 for k in t.tolist()]


def test_the_table_and_the_spellings_through_the_op_and_the_public_calls(pool, vocab, spelled):
    want = agree(pool, vocab, 64, what="pool")
    ids = vocab.encode(pool, 64)
    natoms, atoms, nbonds, bonds, flags, verdict, status, position = mol_normalize(ids.to(torch.int16), vocab, DEV)
    key = mol_key(ids, vocab, DEV, normalize=True)[0]
    raw = mol_key(ids, vocab, DEV)[0]
    fp, count, _, _ = mol_fingerprint(ids, vocab, DEV, normalize=True)
    torch.cuda.synchronize()
    assert all(t.dtype == torch.int64 for t in (natoms, atoms, nbonds, bonds, flags, verdict, status, position))
    assert atoms.tolist() == [r["atoms"] for r in want] and bonds.tolist() == [r["bonds"] for r in want]
    assert flags.tolist() == [r["flags"] for r in want] and verdict.tolist() == [H.string_hydrogens(s)["verdict"] for s in pool]
    assert natoms.tolist() == [r["n"] for r in want] and nbonds.tolist() == [r["nb"] for r in want]
    assert status.tolist() == [S.check(s)[0] for s in pool]
    assert unsigned(key) == [N.normal_key(s) for s in pool] and unsigned(raw) == [K.string_key(s) for s in pool]
    got_fp = [F.from_words(row) for row in fp.tolist()]
    want_fp = [F.fingerprint(*N.unpacked(r)) if r["molecule"] else 0 for r in want]
    assert got_fp == want_fp and count.tolist() == [F.popcount(b) for b in want_fp]
    by = dict(zip(pool, zip(unsigned(key), unsigned(raw), atoms.tolist(), flags.tolist())))
    for s, aromatic in N.TABLE.items():                                      # the hand table, straight from the device
        n = N.string_normal(s)["n"]
        aromatic = set(range(n)) if aromatic == N.ALL else aromatic
        assert {x for x in range(n) if by[s][2][x] >> 10 & 1} == aromatic and by[s][3] & 3 == (3 if aromatic else 1), s
    for a, b in N.PAIRS:                                                     # as written two molecules, as normal forms one
        assert by[a][1] != by[b][1] and by[a][0] == by[b][0] != 0, (a, b)
    at = len(N.TABLE) + 2 * len(N.PAIRS)
    for k, (_, sp) in enumerate(spelled):                                    # the four spellings of a graph: one key
        assert pool[at + 4 * k:at + 4 * k + 4] == sp and len(set(unsigned(key[at + 4 * k:at + 4 * k + 4]))) == 1, sp
    for s in NO_KEKULE + NO_MOLECULE:                                        # passed through: the key as written
        assert by[s][0] == by[s][1] and by[s][3] == 0, s


def test_similarity_and_substructure_on_normal_forms(vocab):
    pairs = [p for p in N.PAIRS if len(p[0]) <= 32 and len(p[1]) <= 32]
    a, b = vocab.encode([p[0] for p in pairs], 32), vocab.encode([p[1] for p in pairs], 32)
    sim, inter, union = tanimoto(a, b, vocab, DEV, normalize=True)
    plain = tanimoto(a, b, vocab, DEV)[0]
    known = KnownSet(a, 32)
    near, index, n_inter, n_union = nearest_known_tanimoto(b, known, vocab, DEV, normalize=True)
    far = nearest_known_tanimoto(b, known, vocab, DEV)[0]
    torch.cuda.synchronize()
    assert torch.equal(inter, union) and sim.tolist() == [1.0] * len(pairs) and (plain < 1).all()
    assert near.tolist() == [1.0] * len(pairs) and torch.equal(n_inter, n_union) and (far < 1).all()
    want = [F.counts(F.fingerprint(*N.unpacked(N.string_normal(p))), F.fingerprint(*N.unpacked(N.string_normal(q)))) for p, q in pairs]
    assert list(zip(inter.tolist(), union.tolist())) == want
    assert [known.packed[i].tolist() for i in index.tolist()] == [vocab.encode([p[0]], 32)[0].tolist() for p in pairs]
    targets = ["C", "[CH4]", "C1=CNC=C1", "c1cc[nH]c1", "C1=CC=CC=C1", "c1ccccc1", "OC1=CC=CC=C1", "C1CCCCC1", "CC", "c1cccc1", "C(", "cc"]
    patterns = ["[CH4]", "[nH]", "c1ccccc1", "C1=CC=CC=C1", "C", "c", "[CH3]", "C=C", "cO"]
    ids = vocab.encode(targets, 16)
    match, undecided, status, _ = has_substructure_normalized(ids, patterns, vocab, DEV)
    old = has_substructure(ids, patterns, vocab, DEV)[0]
    torch.cuda.synchronize()
    p_graphs = [B.graph_of(p) for p in patterns]
    for r, t in enumerate(targets):                                          # molsub_ref's match on the reference's normal form
        form = N.string_normal(t)
        ta, tb = N.unpacked(form) if form["molecule"] else ([], [])
        row = [B.match_arrays(len(ta), ta, len(tb), tb, len(pa), pa, len(pb), pb)[0] == B.MATCH for pa, pb in p_graphs]
        assert match[r].tolist() == row and not undecided[r].any(), t
        assert old[r].tolist() == [B.contains(p, t) for p in patterns], t
    got = {(t, p): bool(match[r, q]) for r, t in enumerate(targets) for q, p in enumerate(patterns)}
    was = {(t, p): bool(old[r, q]) for r, t in enumerate(targets) for q, p in enumerate(patterns)}
    assert got["C", "[CH4]"] and not was["C", "[CH4]"] and got["[CH4]", "[CH4]"] and not got["CC", "[CH4]"] and got["CC", "[CH3]"]
    assert got["C1=CNC=C1", "[nH]"] and not was["C1=CNC=C1", "[nH]"] and got["c1cc[nH]c1", "[nH]"]
    assert got["C1=CC=CC=C1", "c1ccccc1"] and not was["C1=CC=CC=C1", "c1ccccc1"] and got["OC1=CC=CC=C1", "cO"]
    assert not got["C1=CC=CC=C1", "C1=CC=CC=C1"] and was["C1=CC=CC=C1", "C1=CC=CC=C1"]        # aromatic fragments: lower case
    assert not got["C1CCCCC1", "c"] and got["cc", "C=C"] and not got["cc", "c"] and not got["C(", "C"]
    assert got["c1cccc1", "c"] and not got["c1cccc1", "C"]                   # no Kekule structure: matched as written


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 67])
@pytest.mark.parametrize("L", [1, 33, 64])
def test_row_shapes(L, R_, pool, vocab):
    """Molecule rows interleaved with empty rows and rows of status != 0, cut to the width (some become no molecule: a case)."""
    rng = np.random.default_rng(100 * L + R_)
    if L == 1:
        strings = [["c", "C", "*", "", "(", "N", "F", "O"][int(rng.integers(8))] for _ in range(R_)]
    else:
        strings = [["", "C(", pool[int(rng.integers(len(pool)))][:L]][min(int(rng.integers(6)), 2)] for _ in range(R_)]
    agree(strings, vocab, L, what=(L, R_))


def test_no_rows_launches_nothing(vocab):
    n, rows, h, v = (torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV),
                     torch.zeros(0, 8, dtype=torch.uint8, device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV))
    out = torch.ops.mdt.mol_normalize(n, rows, n, rows, h, h, v, h)
    assert [tuple(t.shape) for t in out] == [(0, 8), (0, 8), (0,)]
    out = mol_normalize(torch.zeros(0, 8, dtype=torch.long), vocab, DEV)
    assert out[1].shape == (0, 8) and out[4].shape == (0,)
    assert mol_key(torch.zeros(0, 8, dtype=torch.long), vocab, DEV, normalize=True)[0].shape == (0,)


def test_full_width_rows(vocab):
    strings = ["c" * 64, "c1ccccc1" * 8, "C" * 64, "C1=CC=CC=C1" * 5 + "CCCCCCCCC", "[nH]1cccc1" * 6 + "cccc", "*" * 64, "", "C(",
               "c1ccc2ccccc2c1" * 4 + "c1ccccc1", "C1" + "C" * 60 + "C1", "N" * 63 + "O"]
    assert all(len(s) <= 64 for s in strings) and len(strings[0]) == len(strings[1]) == len(strings[3]) == 64
    want = agree(strings, vocab, 64, what="full width")
    chain = N.unpacked(want[0])                                              # kekulisable, no ring: de-aromatised, lane 63 in use
    assert want[0]["flags"] == N.NORMALIZED | N.CHANGED and want[0]["n"] == 64 and not any(d >> 10 & 1 for d in chain[0])
    assert sorted(o for _, _, o in chain[1]) == [1] * 31 + [2] * 32 and chain[1][62][:2] == (62, 63)
    assert want[1]["flags"] == 7 and want[1]["n"] == 48 and len(want[1]["aromatic"]) == 48 and len(want[1]["rings"]) == 8
    assert [o for _, _, o in N.unpacked(want[1])[1]].count(5) == 48
    assert want[2]["flags"] == N.NORMALIZED and want[3]["flags"] == 7 and len(want[3]["aromatic"]) == 30
    assert want[5]["flags"] == N.NORMALIZED and want[8]["flags"] & N.AROMATIC and len(want[8]["aromatic"]) == 46


def test_graph_arrays_that_no_scan_writes():
    """A 62-ring of alternating bonds is aromatic (31 search levels), a 64-ring is not; entries listed twice, entries (x, x), orders
    outside 1..5, hydrogens no rule gives (the H field clamps at 15), a ring size the search cannot confirm, a verdict handed in, and
    counts outside the row."""
    special = N.special_rows()
    W = 64
    rows = [row for row, _ in special]
    natoms = torch.tensor([row[1] for row in rows], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([row[2] for row in rows], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(rows), W), 0x7FFFFFFF, dtype=torch.int32, device=DEV)    # (beyond the counts: never read)
    bonds = torch.full((len(rows), W), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    hydrogens = torch.full((len(rows), W), 0xA5, dtype=torch.uint8, device=DEV)
    partner = torch.full((len(rows), W), 0xA5, dtype=torch.uint8, device=DEV)
    bond_ring = torch.full((len(rows), W), 0xA5, dtype=torch.uint8, device=DEV)
    verdict = torch.tensor([row[7] for row in rows], dtype=torch.uint8, device=DEV)
    for r, (_, _, _, la, lb, lh, lp, _, lr) in enumerate(rows):
        if la:
            atoms[r, :len(la)] = torch.tensor(la, dtype=torch.int32)
            hydrogens[r, :len(la)] = torch.tensor(lh, dtype=torch.uint8)
            partner[r, :len(la)] = torch.tensor(lp, dtype=torch.uint8)
        if lb:
            words = [N.pack(e) for e in lb]
            bonds[r, :len(lb)] = torch.tensor([w - (1 << 32 if w >> 31 else 0) for w in words], dtype=torch.int32)
            bond_ring[r, :len(lb)] = torch.tensor(lr, dtype=torch.uint8)
    want = [N.normalize_arrays(n, la, nb, lb, lh, lp, v, lr, W) for (_, n, nb, la, lb, lh, lp, v, lr) in rows]
    for r, (_, named) in zip(want, special):
        assert r["flags"] == named["flags"] and r["aromatic"] == named.get("aromatic", r["aromatic"])
    assert want[0]["aromatic"] == set(range(62)) and want[1]["aromatic"] == set() and want[6]["atoms"][0] >> 17 & 15 == 15
    got = torch.ops.mdt.mol_normalize(natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring)
    agree_arrays(got, want)


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry point on outputs pre-filled by poison_util (NaN bits, then large garbage), each followed by a guard band of the same
    fill: every output word comes out defined, zero beyond the counts, and the guard comes back as it was."""
    strings = pool[::9] + NO_MOLECULE + NO_KEKULE + ["c" * 64, "c1ccccc1" * 8]
    for L, fill in ((64, P.NAN), (37, P.GARBAGE)):
        rows = [s[:L] for s in strings]
        inputs = op_inputs(rows, vocab, L)
        R_ = len(rows)
        guard = 64                                                           # words of the fill after each output
        sizes = [(R_ * L, torch.int32, (R_, L)), (R_ * L, torch.int32, (R_, L)), (R_, torch.uint8, (R_,))]
        raw, out, before = [], [], []
        for seed, (count, dtype, shape) in enumerate(sizes):
            words = (count + 3) // 4 if dtype == torch.uint8 else count
            image = P.fill_bits(fill, words + guard, seed, DEV)
            raw.append(image)
            before.append(image.clone())
            out.append(image.view(dtype)[:count].view(shape))
        with torch.cuda.device(DEV):
            rt.check(rt.load_library().mdt_mol_normalize(*[rt.ptr(t) for t in inputs], L, R_, *[rt.ptr(t) for t in out],
                                                         rt.current_stream()))
        want = [N.string_normal(s, L) for s in rows]
        agree_arrays(out, want, what=L)
        assert 0 < sum(r["flags"] != 0 for r in want) < len(want) and sum(r["flags"] >> 1 & 1 for r in want) > 20
        beyond_atoms = torch.arange(L, device=DEV).unsqueeze(0) >= inputs[0].long().unsqueeze(1)
        beyond_bonds = torch.arange(L, device=DEV).unsqueeze(0) >= inputs[2].long().unsqueeze(1)
        assert not out[0][beyond_atoms].any() and not out[1][beyond_bonds].any()
        for image, was, (count, dtype, _) in zip(raw, before, sizes):        # what lies after the outputs is nobody's
            nbytes = count * (1 if dtype == torch.uint8 else 4)
            assert torch.equal(image.view(torch.uint8)[nbytes:], was.view(torch.uint8)[nbytes:])


def test_the_same_call_twice_gives_identical_bits(pool, vocab):
    inputs = op_inputs(pool, vocab, 64)
    first = torch.ops.mdt.mol_normalize(*inputs)
    second = torch.ops.mdt.mol_normalize(*inputs)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_the_normal_form_of_a_normal_form_is_itself_on_the_device(pool, vocab):
    natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring = op_inputs(pool, vocab, 64)
    once = torch.ops.mdt.mol_normalize(natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring)
    h2, p2, v2, _, _ = torch.ops.mdt.mol_hydrogens(natoms, once[0], nbonds, once[1], H.MAX_STEPS)
    ring2 = torch.ops.mdt.mol_rings(natoms, once[0], nbonds, once[1], h2, None, None)[0]
    twice = torch.ops.mdt.mol_normalize(natoms, once[0], nbonds, once[1], h2, p2, v2, ring2)
    torch.cuda.synchronize()
    done = (once[2] & 1).bool()
    assert done.sum() > 1800 and not v2[done].any()
    assert torch.equal(twice[0][done], once[0][done]) and torch.equal(twice[1][done], once[1][done])
    assert torch.equal(twice[2][done], once[2][done] & 3)                    # nothing differs from what was written any more


def test_screening_with_normalize_end_to_end():
    """Three targets, six candidates each on the small model of the graph-identity test.  A group holding c1ccccc1O and OC1=CC=CC=C1
    keeps both as written; under normalize=True the second gets bit 4.  A known set holding the aromatic spelling gives the Kekule
    candidate bit 8.  forbid=["c1ccccc1"] rejects the Kekule spelling only under normalize=True.  normalize=False returns what the
    call returns without the keyword, bit for bit."""
    G2, N2, K2, L2, T = 3, 6, 6, 32, 4
    vocab = SmilesVocabulary([None] + list("CNOcno14()-=#[H]"))
    order = [["c1ccccc1O", "CCO", "OC1=CC=CC=C1", "CC(=O)N", "C1CCCCC1O", "Oc1ccccc1"],
             ["CCN", "C1=CNC=C1", "C(", "c1cc[nH]c1", "C1=CC=CC=C1", "OCCO"],
             ["C", "[CH4]", "C1CC1", "O", "N1CCCC1", "C1=CC=NC=C1"]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]            # row c * G + g
    tokens = vocab.encode(strings, L2)
    known = KnownSet(vocab.encode(["c1ccncc1", "CCCC"], L2), L2)
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, vocabulary=vocab, identity="graph", known_tokens=known)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    run = lambda **more: screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, forward_noise=noise(), **kw, **more)  # noqa: E731
    plain, off, on, again = run(), run(normalize=False), run(normalize=True), run(normalize=True)
    ban, ban_on = run(forbid=["c1ccccc1"]), run(forbid=["c1ccccc1"], normalize=True)
    full = run(normalize=True, kekulize=True, limits=None, max_similarity=1.0)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # False: today's result, field for field; and repeatable
        for a, b in ((getattr(off, name), getattr(plain, name)), (getattr(again, name), getattr(on, name))):
            assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    st = lambda out, g: dict(zip(order[g], out.status[:, g].tolist()))  # noqa: E731
    assert st(plain, 0)["OC1=CC=CC=C1"] & 12 == 0 and st(on, 0)["OC1=CC=CC=C1"] & 12 == 4     # phenol, written twice
    assert st(plain, 0)["Oc1ccccc1"] & 4 == 4 and st(on, 0)["Oc1ccccc1"] & 4 == 4 and st(on, 0)["c1ccccc1O"] & 12 == 0
    assert st(plain, 1)["c1cc[nH]c1"] & 4 == 0 and st(on, 1)["c1cc[nH]c1"] & 4 == 4 and st(on, 1)["C1=CNC=C1"] & 4 == 0
    assert st(plain, 2)["[CH4]"] & 4 == 0 and st(on, 2)["[CH4]"] & 4 == 4                     # methane, written twice
    assert st(plain, 2)["C1=CC=NC=C1"] & 8 == 0 and st(on, 2)["C1=CC=NC=C1"] & 8 == 8         # known in the aromatic spelling
    kept = lambda out, g: [order[g][c] for c in out.index[g].tolist() if c >= 0]  # noqa: E731
    assert "OC1=CC=CC=C1" in kept(plain, 0) and "OC1=CC=CC=C1" not in kept(on, 0) and "c1ccccc1O" in kept(on, 0)
    assert "[CH4]" not in kept(on, 2) and "C1=CC=NC=C1" not in kept(on, 2) and "C" in kept(on, 2)
    assert st(ban, 1)["C1=CC=CC=C1"] & 128 == 0 and st(ban_on, 1)["C1=CC=CC=C1"] & 128 == 128  # the Kekule spelling of the banned ring
    assert st(ban, 0)["c1ccccc1O"] & 128 == 128 and st(ban_on, 0)["c1ccccc1O"] & 128 == 128 and st(ban_on, 0)["CCO"] & 128 == 0
    assert st(ban, 0)["OC1=CC=CC=C1"] & 128 == 0 and st(ban_on, 0)["OC1=CC=CC=C1"] & 128 == 128
    want = {s: 4 * (N.normal_key(s) in {N.normal_key(t) for t in order[g][:c]}) | 8 * (N.normal_key(s) in {N.normal_key("c1ccncc1"), N.normal_key("CCCC")})
            for g in range(G2) for c, s in enumerate(order[g]) if N.normal_key(s)}
    for g in range(G2):                                                      # bits 4 and 8 by the reference's normal-form keys
        for s, status in st(on, g).items():
            if s in want:
                assert status & 12 == want[s], s
    for g in range(G2):                                                      # similarity 1.0 on normal forms: no second phenol kept
        assert len({N.normal_key(s) for s in kept(full, g)}) == len(kept(full, g))
