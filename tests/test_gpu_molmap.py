"""-m gpu: mdt_sub_map (csrc/k_molsub.hip, k_sub_map), substructure_map(), substructure_keep(), SubstructureCounts and the
screening call with ``counts=`` on the device.  Every comparison is exact: every found, capped, embeddings, cover and map word and
every flag against the plain-int reference tests/molmap_ref.py (whose graphs are tests/molkey_ref.py's), and on every row of
every test mdt_sub_match's two words against what ``found`` / ``capped`` imply.  No row here can run longer than its step cap: at
most 64 roots of 4,096 steps per (row, pattern), and once more for the one root whose first map is handed out."""
import functools

import numpy as np
import pytest
import torch

import molkey_ref as K
import molmap_ref as A
import molscaf_ref as C
import molsub_ref as B
import molwrite_ref as W
import poison_util as P
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, SubstructureCounts, SubstructureSet, has_substructure,
                                              runtime as rt, screen_tokens_diverse, substructure_keep, substructure_map)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

RING_SYSTEM = "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3"              # (as the graph key's full-width test)
RING_MAX = "*" + "0123456789" + ("*" + "0123456789" * 2) * 2 + "*" + "0123456789"     # 64 tokens, 4 atoms, 30 ring bonds
CAP_PATTERN, CAP_UNDECIDED, CAP_MATCH = "C.C.C.C.C.C.CN", "C" * 62 + ".N", "C" * 61 + "CN"
ROWS_PER_BLOCK = 4                                                          # k_sub_map: waves (rows in flight) of a workgroup
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def vocab(spelled):
    chars = set(S.CHARS) | set("".join(s for _, sp in spelled for s in sp)) | set("$:*%\\/")
    return SmilesVocabulary([None] + sorted(chars))


@pytest.fixture(scope="module")
def pool(spelled):
    """test_gpu_molsub.py's pool: strings of at most 64 tokens, spellings, and mutated rows of which most are no molecule."""
    rng = np.random.default_rng(5)
    broken = [s[:int(rng.integers(1, len(s) + 1))] + ("(" if r % 3 else "") for r, s in enumerate(S.mutated_rows(256)) if s]
    assert sum(not B.graph_of(s)[0] for s in broken) > 0.5 * len(broken)
    return [s for _, sp in spelled[:60] for s in sp] + broken


@functools.lru_cache(maxsize=None)
def reference(pattern, target, L, LP):
    w = A.string_map(pattern, target, L, LP)
    return w["found"], w["capped"], w["embeddings"], w["cover"], tuple(w["map"])


def graph_arrays(strings, vocabulary, width):
    """The graph arrays of mdt::mol_graph, int32 on the device; a string that is no molecule has no atoms."""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    return torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]


def unsigned(t):
    return [[int(x) & MASK64 for x in row] for row in t.tolist()]


def compare(got, targets, patterns, L, LP, lo=None, hi=None, what=None):
    """The six outputs of mdt::sub_map against the reference, word for word -> the reference's rows"""
    found, capped, embeddings, cover, fmap, flags = got
    R_, P_ = len(targets), len(patterns)
    assert [(t.dtype, tuple(t.shape)) for t in got] == [(torch.int64, (R_, P_)), (torch.int64, (R_, P_)), (torch.int32, (R_, P_)),
                                                        (torch.int64, (R_, P_)), (torch.uint8, (R_, P_, LP)), (torch.uint8, (R_,))]
    want = [[reference(p, t, L, LP) for p in patterns] for t in targets]
    got_words = list(zip(unsigned(found), unsigned(capped), embeddings.tolist(), unsigned(cover), fmap.tolist()))
    for r, t in enumerate(targets):
        for q, p in enumerate(patterns):
            one = tuple(x[q] for x in got_words[r][:4]) + (tuple(got_words[r][4][q]),)
            assert one == want[r][q], (what, r, t, q, p)
    if lo is None:
        assert not flags.any()
    else:
        assert flags.tolist() == [A.count_flag([w[0] for w in row], [w[1] for w in row], lo, hi) for row in want], what
    return want


def agree(targets, patterns, vocabulary, L, LP, seed=0, what=None):
    """mdt::sub_map with random bounds against the reference, and mdt::sub_match against what found / capped imply"""
    tg, pg = graph_arrays(targets, vocabulary, L), graph_arrays(patterns, vocabulary, LP)
    rng = np.random.default_rng(seed)
    lo = [int(x) for x in rng.choice([0, 0, 0, 1, 2], len(patterns))]
    hi = [int(x) for x in rng.choice([0, 1, 3, 63, 64, 255], len(patterns))]
    bounds = [torch.tensor(b, dtype=torch.uint8, device=DEV) for b in (lo, hi)]
    got = torch.ops.mdt.sub_map(*tg, *pg, *bounds)
    match, undecided, _ = torch.ops.mdt.sub_match(*tg, *pg, 0, 0)
    torch.cuda.synchronize()
    want = compare(got, targets, patterns, L, LP, lo, hi, what)
    bits = lambda word: word.cpu().numpy().view(np.uint32).tolist()  # noqa: E731
    assert bits(match) == [sum(1 << q for q, w in enumerate(row) if w[0]) for row in want], what
    assert bits(undecided) == [sum(1 << q for q, w in enumerate(row) if not w[0] and w[1]) for row in want], what
    return want


def patterns_of(P_, LP, seed):
    rng = np.random.default_rng(seed)
    source = B.PATTERNS + B.EVERYDAY + ["CC(C)C", "OCC", "C1CC1C", "*C", "C(C1)1", "[nH]", "Cl", "C(", ""]
    return [source[int(rng.integers(len(source)))][:LP] for _ in range(P_)]  # (cut short: some are no molecule, which is a case)


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 257])
@pytest.mark.parametrize("L", [1, 33, 64])
def test_sub_map_row_shapes(L, R_, pool, vocab):
    rng = np.random.default_rng(100 * L + R_)
    targets = [pool[int(rng.integers(len(pool)))][:L] for _ in range(R_)]
    P_, LP = [(1, 17), (31, 32), (32, 1), (32, 32), (31, 17)][(L + R_) % 5]
    agree(targets, patterns_of(P_, LP, R_), vocab, L, LP, seed=R_, what=(L, R_, P_, LP))


@pytest.mark.parametrize("P_", [1, 31, 32])
@pytest.mark.parametrize("LP", [1, 17, 32])
def test_sub_map_pattern_shapes(LP, P_, pool, vocab):
    targets = pool[:40:3] + pool[-6:]
    want = agree(targets, patterns_of(P_, LP, 7 * P_ + LP), vocab, 64, LP, seed=P_, what=(P_, LP))
    assert P_ == 1 or (any(w[0] for row in want for w in row) and not all(w[0] for row in want for w in row))
    assert LP == 1 or P_ == 1 or any(w[2] > bin(w[0]).count("1") for row in want for w in row)     # more maps than anchors somewhere


def test_the_high_half_of_the_words(vocab):
    """Targets whose only root is atom 40 or higher, and maps that reach across bit 32"""
    targets = ["C" * 40 + "N", "C" * 63 + "N", "N" + "C" * 63, "C" * 31 + "NC" + "C" * 30 + "O", "C" * 64, "C(C)(C)CO"]
    want = agree(targets, ["NC", "CCO", "N", "OC", "C(C)(C)(C)CCO", "CNC"], vocab, 64, 32, what="roots")
    assert want[0][0][:4] == (1 << 40, 0, 1, 3 << 39) and want[0][0][4][:2] == (41, 40)
    assert want[1][0][:4] == (1 << 63, 0, 1, 3 << 62) and want[1][0][4][:2] == (64, 63)
    assert want[3][3][0] == 1 << 63 and want[3][5][0] == (1 << 30) | (1 << 32) and want[3][5][3] == 7 << 30
    assert want[4][1][0] == 0 and want[5][1][:3] == (0b00001, 0, 1)


def test_full_width_rows_and_patterns(vocab):
    """The rows of test_gpu_molsub.py::test_full_width_rows_and_patterns, the two cap rows included"""
    targets = ["C" * 64, RING_MAX, RING_SYSTEM, "C1" * 32, "c1ccccc1" * 8, "*" * 64, "", "C(", CAP_UNDECIDED, CAP_MATCH]
    patterns = ["C" * 32, "*" * 32, "c1ccccc1c1ccccc1", "C1CCCCCCCCCCCCCCC1", "C(C)(C)C", "*.*.*.*", CAP_PATTERN, "C", "cc"]
    assert len(RING_MAX) == 64 and all(len(t) <= 64 for t in targets) and all(len(p) <= 32 for p in patterns)
    want = agree(targets, patterns, vocab, 64, 32, seed=3, what="full width")
    none, some = want[8][6], want[9][6]                                      # the two cap rows: nothing found, 61 anchors found
    assert none[:4] == (0, (1 << 62) - 1, 0, 0) and some[0] == (1 << 61) - 1 and some[1] == (1 << 62) - 1 and some[4][:8] == (1, 2, 3, 4, 5, 6, 62, 63)
    assert sum(1 for row in want for w in row if w[1]) >= 6 and want[0][7][:4] == (MASK64, 0, 64, MASK64)
    assert all(w == (0, 0, 0, 0, (0,) * 32) for r in (6, 7) for w in want[r])               # the rows that are no molecule
    out = substructure_map(vocab.encode(targets, 64), SubstructureSet(patterns, vocab), vocab, DEV)
    torch.cuda.synchronize()
    assert out.count.tolist() == [[bin(w[0]).count("1") for w in row] for row in want]
    assert out.undecided.tolist() == [[w[1] != 0 for w in row] for row in want] and out.embeddings.tolist() == [[w[2] for w in row] for row in want]
    assert out.atom_map.tolist() == [[list(w[4]) for w in row] for row in want]
    for name, k in (("found", 0), ("cover", 3)):
        assert getattr(out, name).tolist() == [[[bool(w[k] >> t & 1) for t in range(64)] for w in row] for row in want], name
    assert out.status.tolist() == [S.check(t)[0] for t in targets] and out.position.tolist()[7] == 2
    match, undecided, _, _ = has_substructure(vocab.encode(targets, 64), patterns, vocab, DEV)
    assert torch.equal(match, out.count > 0) and torch.equal(undecided, (out.count == 0) & out.undecided)


def test_graph_arrays_that_no_scan_writes_and_no_rows(vocab):
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
    found, capped, embeddings, cover, fmap, flags = torch.ops.mdt.sub_map(natoms, atoms, nbonds, bonds, natoms, atoms, nbonds, bonds, None, None)
    torch.cuda.synchronize()
    want = [[A.map_arrays(n, [c] * 8, nb, tb, m, [c] * 8, mb, pb, 8, 8) for m, mb, pb in odd] for n, nb, tb in odd]
    for name, got in (("found", unsigned(found)), ("capped", unsigned(capped)), ("embeddings", embeddings.tolist()), ("cover", unsigned(cover)),
                      ("map", fmap.tolist())):
        assert got == [[w[name] for w in row] for row in want], name
    assert not any(w["found"] for row in want[:5] for w in row) and want[11][9]["embeddings"] == 6 and want[8][8]["found"] == 0b01 and want[8][8]["map"][:2] == [1, 2]
    empty = torch.ops.mdt.sub_map(natoms[:0], atoms[:0], nbonds[:0], bonds[:0], natoms, atoms, nbonds, bonds, None, None)
    assert [tuple(t.shape) for t in empty] == [(0, 12), (0, 12), (0, 12), (0, 12), (0, 12, 8), (0,)]


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry point on outputs pre-filled with garbage, with NaN bits and with zeros, each followed by a guard band of the same
    fill: the three results are identical and the reference's, and the guard comes back as it was."""
    targets = [s[:37] for s in pool[::7]] + ["", "C(", "C" * 37]
    patterns = patterns_of(9, 17, 3) + ["C.C.C.C.C.C", ""]
    L, LP, R_, P_ = 37, 17, len(targets), 11
    inputs = graph_arrays(targets, vocab, L) + graph_arrays(patterns, vocab, LP)
    lo, hi = [0] * 11, [2, 64, 3] * 3 + [64, 255]
    bounds = [torch.tensor(b, dtype=torch.uint8, device=DEV) for b in (lo, hi)]
    sizes = [(R_ * P_, torch.int64), (R_ * P_, torch.int64), (R_ * P_, torch.int32), (R_ * P_, torch.int64), (R_ * P_ * LP, torch.uint8),
             (R_, torch.uint8)]
    shapes = [(R_, P_)] * 4 + [(R_, P_, LP), (R_,)]
    results = []
    for fill in (P.GARBAGE, P.NAN, P.ZERO):
        raw, before, out, guard = [], [], [], 64
        for seed, ((count, dtype), shape) in enumerate(zip(sizes, shapes)):
            nbytes = count * torch.empty(0, dtype=dtype).element_size()
            image = P.fill_bits(fill, (nbytes + 3) // 4 + guard, seed, DEV)
            raw.append(image)
            before.append(image.clone())
            out.append(image.view(torch.uint8)[:nbytes].view(dtype).view(shape))
        lib = rt.load_library()
        with torch.cuda.device(DEV):
            rt.check(lib.mdt_sub_map(*[rt.ptr(t) for t in inputs[:4]], L, R_, *[rt.ptr(t) for t in inputs[4:]], LP, P_,
                                     *[rt.ptr(t) for t in bounds], *[rt.ptr(t) for t in out], rt.current_stream()))
        torch.cuda.synchronize()
        compare(out, targets, patterns, L, LP, lo, hi, fill)
        for image, was, (count, dtype) in zip(raw, before, sizes):           # what lies after the outputs is nobody's
            nbytes = count * torch.empty(0, dtype=dtype).element_size()
            assert torch.equal(image.view(torch.uint8)[nbytes:], was.view(torch.uint8)[nbytes:]), fill
        results.append([t.clone() for t in out])
    assert all(torch.equal(a, b) for other in results[1:] for a, b in zip(results[0], other))
    assert results[0][5].any() and not results[0][5].all() and results[0][1].any()          # flags both ways, and a capped root


def keep_reference(strings, patterns, table, W_, occurrences, normalize):
    """substructure_keep() from molwrite_ref and molmap_ref: the row written from the graph as written, the match on the graph as
    written or on its normal form -> (written rows, masks, matched, complete)"""
    fragments = [B.graph_of(p) for p in patterns]
    rows, masks, matched, complete = [], [], [], []
    for s in strings:
        graph, read = C.input_arrays(s), C.input_arrays(s, normalize)
        row = W.write_arrays(*graph, W.priority(*graph, 64), table, W_)
        words = [A.map_arrays(*read, len(pa), pa, len(pb), pb) for pa, pb in fragments]
        atoms = set()
        for w in words:
            atoms |= {t for t in range(64) if w["cover"] >> t & 1} if occurrences == "all" else {b - 1 for b in w["map"] if b}
        rows.append(row)
        masks.append([o != 0 and o - 1 in atoms for o in row["token_atom"]])
        matched.append([w["found"] != 0 for w in words])
        complete.append(all(w["capped"] == 0 for w in words))
    return rows, masks, matched, complete


def test_substructure_keep(spelled, vocab):
    strings = [sp[k % 4] for k, (_, sp) in enumerate(spelled[:40])] + ["CC(=O)Nc1ccccc1", "C1=CC=CC=C1C", "", "C(", "FC(F)(F)C(F)(F)F", CAP_MATCH]
    patterns = ["C(=O)", "c1ccccc1", "N", "C(F)(F)F", "CC", CAP_PATTERN]
    ids, table = vocab.encode(strings, 64), W.class_table(vocab.chars)
    for occurrences, normalize, width in (("all", False, None), ("first", False, 80), ("all", True, None), ("first", True, 64)):
        W_ = width or 64
        tokens, keep, matched, complete, flags, status, position = substructure_keep(ids, patterns, vocab, DEV, occurrences=occurrences,
                                                                                     normalize=normalize, width=width)
        torch.cuda.synchronize()
        rows, masks, want_matched, want_complete = keep_reference(strings, patterns, table, W_, occurrences, normalize)
        assert keep.dtype == matched.dtype == complete.dtype == torch.bool and tokens.dtype == flags.dtype == torch.int64
        assert tokens.tolist() == [r["tokens"] for r in rows] and flags.tolist() == [r["flags"] for r in rows], (occurrences, normalize)
        assert keep.tolist() == masks and matched.tolist() == want_matched and complete.tolist() == want_complete, (occurrences, normalize)
        assert status.tolist() == [S.check(s)[0] for s in strings]
        assert sum(any(m) for m in masks) >= 30 and not any(masks[42]) and not any(masks[43]) and complete.tolist()[-1] is False
    all_mask = substructure_keep(ids, ["C(F)(F)F"], vocab, DEV)[1][44]           # "all" keeps both CF3 groups, "first" one
    first_mask = substructure_keep(ids, ["C(F)(F)F"], vocab, DEV, occurrences="first")[1][44]
    assert int(all_mask.sum()) > int(first_mask.sum()) > 0 and bool((all_mask | ~first_mask).all())
    # c1ccccc1 is kept in C1=CC=CC=C1C only through the normal form, and the lead stays as written either way
    for normalize in (False, True):
        tokens, keep, matched = substructure_keep(vocab.encode(["C1=CC=CC=C1C"], 64), ["c1ccccc1"], vocab, DEV, normalize=normalize)[:3]
        text = vocab.decode(tokens)[0]
        kept = "".join(ch for ch, k in zip(text, keep[0].tolist()) if k)
        assert matched.tolist() == [[normalize]] and text.count("C") == 7 and text.count("=") == 3 and "[" not in text and "c" not in text
        assert kept.count("C") == (6 if normalize else 0) and kept.count("=") == (3 if normalize else 0), (text, kept)


def test_refining_a_lead_around_a_matched_fragment():
    """substructure_keep()'s mask fed to refine_keep_tokens() on the tiny model: every kept position of the output is the lead's id"""
    m = make_model("tiny")                                                   # 16 ids, rows of 32 positions
    vocab = SmilesVocabulary([None] + list("CNOcno1()-=#[H]"))
    leads = ["CC(=O)Nc1ccccc1", "OC(=O)CCN", "OCC", "NC1CC1C(=O)O", "C(", "O=C1CCC1CN", "C1=CC=CC=C1C(=O)N"]
    assert len(vocab) == 15 == m.pred_dim - 1 and m.max_length == 32
    tokens, keep, matched, complete, flags, status, _ = substructure_keep(vocab.encode(leads, 32), ["C(=O)N", "C(=O)O"], vocab, DEV)
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 1, 1, 1, 0, 1, 1] and complete.all() and not keep[4].any() and not keep[2].any()
    assert matched.tolist() == [[True, False], [False, True], [False, False], [False, True], [False, False], [False, False], [True, False]]
    seq = synth_normal("molmap/seq", (len(leads), 12))
    for start in (2, [0, 5, 3, 1, 4, 2, 6]):
        out = m.refine_keep_tokens(seq, DEV, tokens.cpu(), start_step=start, cond_scale=2.0, timesteps=8, noise=NoiseSource(seed=17),
                                   keep_mask=keep.cpu())
        torch.cuda.synchronize()
        assert out.shape == tokens.shape and torch.equal(out[keep], tokens[keep]) and int(keep.sum()) >= 12


def test_screening_with_counts_end_to_end():
    """Four targets, eight candidates each on the small model of the substructure screening test: a kept candidate has exactly one
    carbonyl carbon and at most one nitrogen.  Bit 128 sits where the reference says, kept rows never carry it, and they are the
    best of the rest."""
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
    patterns, lo, hi = ["C=O", "N"], [1, 0], [1, 1]
    counts = SubstructureCounts(patterns, vocab, at_least=[1, None], at_most=[1, 1])
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, counts=counts, forward_noise=noise(), **kw)
    plain = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, forward_noise=noise(), **kw)
    none = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, counts=None, forward_noise=noise(), **kw)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # None: today's result, field for field
        a, b = getattr(none, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    words = [[A.string_map(p, s, 32, 32) for p in patterns] for s in strings]
    flagged = np.array([A.count_flag([w["found"] for w in row], [w["capped"] for w in row], lo, hi) for row in words],
                       dtype=np.uint8).reshape(N2, G2)
    assert flagged[:, 2].all() and not flagged[:7, 3].all() and flagged[5, 3] and flagged[4, 3] and 0 < flagged.sum() // 128 < 32
    want = plain.status.cpu().numpy() | flagged
    assert out.status.dtype == torch.uint8 and np.array_equal(out.status.cpu().numpy(), want)
    index = [[c for c in plain.index[g].tolist() if c >= 0 and not flagged[c, g]][:K2] for g in range(G2)]
    count = [len(kept) for kept in index]
    assert out.index.tolist() == [kept + [-1] * (K2 - len(kept)) for kept in index] and out.count.tolist() == count and count[2] == 0
    assert all(want[c, g] & 128 == 0 for g in range(G2) for c in index[g]) and sum(count) >= 6
