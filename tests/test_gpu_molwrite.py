"""-m gpu: mdt_mol_rank / mdt_mol_write (csrc/k_molwrite.hip), mol_write(), mol_respell(), scaffold_tokens() and scaffold_keep() on
the device.  Every comparison is exact: the priority, the tokens, the length, token_atom and the flags against the plain-int
reference tests/molwrite_ref.py on the graphs of tests/molkey_ref.py, the normal forms of tests/molnorm_ref.py and the scaffolds of
tests/molscaf_ref.py.  No row here can run long: n compares, three passes over the entries and two walks of at most 2 n and n + nb
steps a row."""
import numpy as np
import pytest
import torch

import molh_ref as H
import molkey_ref as K
import molnorm_ref as N
import molscaf_ref as C
import molwrite_ref as W
import poison_util as P
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, mol_respell, mol_write, runtime as rt, scaffold_keep,
                                              scaffold_tokens)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 4                                                          # k_mol_write: waves (rows) of a workgroup
NO_MOLECULE = ["", "C(", "C1CC", "C=C=C=O=C", "c1ccccc", "Xx"]
LONG = ["C" * 64, "C1CC1" + "C" * 59, "C1CC1" + "C" * 54 + "C1CC1", "C1" + "C" * 60 + "C1", "c1ccccc1" * 8, "O=C1C(=O)C(=O)C1=O"]
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def pool(spelled):
    """The pool of test_gpu_molscaf.py: the 2,000 random spellings, 128 mutated rows, the tables of the normal form and of the
    scaffold, rows that are no molecule and the longest walks: strings of at most 64 tokens."""
    rows = [s for _, sp in spelled for s in sp] + [s[:64] for s in S.mutated_rows(128)] + list(N.TABLE) + list(C.TABLE)
    rows += NO_MOLECULE + LONG
    assert all(len(s) <= 64 for s in rows)
    return rows


@pytest.fixture(scope="module")
def vocab(pool):
    return SmilesVocabulary([None] + sorted(set(S.CHARS) | set("".join(pool)) | set("$:*%\\/csnopbBPSI")))


def table_of(vocabulary):
    return W.class_table(vocabulary.chars)


def graph_of(strings, vocabulary, width, normalize=False):
    """-> the four graph arrays on the device, as written or as normal forms, by the launches that come before mdt::mol_write"""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]
    if normalize:
        hydrogens, partner, verdict, _, _ = torch.ops.mdt.mol_hydrogens(*graph, H.MAX_STEPS)
        bond_ring = torch.ops.mdt.mol_rings(*graph, hydrogens, None, None)[0]
        atoms, bonds, _ = torch.ops.mdt.mol_normalize(*graph, hydrogens, partner, verdict, bond_ring)
        graph = (graph[0], atoms, graph[2], bonds)
    return graph


def device_arrays(rows, width):
    """rows: [(n, atoms, nb, bonds as (a, b, order))] -> the four graph arrays on the device, garbage beyond the lists"""
    natoms = torch.tensor([r[0] for r in rows], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([r[2] for r in rows], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(rows), width), 0x7FFFFFFF, dtype=torch.int32)   # (beyond the counts: never read)
    bonds = torch.full((len(rows), width), 0x7FFFFFFF, dtype=torch.int32)
    signed = lambda w: w - (1 << 32 if w >> 31 else 0)  # noqa: E731
    for r, (_, la, _, lb) in enumerate(rows):
        if la:
            atoms[r, :len(la)] = torch.tensor([signed(w) for w in la], dtype=torch.int32)
        if lb:
            bonds[r, :len(lb)] = torch.tensor([signed(N.pack(e)) for e in lb], dtype=torch.int32)
    return natoms, atoms.to(DEV), nbonds, bonds.to(DEV)


_PRIORITY = {}


def priority_of(n, atoms, nb, bonds, width):
    at = (n, tuple(atoms), nb, tuple(bonds), width)
    if at not in _PRIORITY:
        _PRIORITY[at] = W.priority(n, atoms, nb, bonds, width)
    return _PRIORITY[at]


def agree(graph, rows, table, width, what, widths=(64, 128), invariants=(True, False)):
    """graph: device arrays; rows: the same rows for the reference.  mdt::mol_rank and mdt::mol_write against the reference, at every
    width, with and without the priority.  -> the reference's answers at the first width with the first of `invariants`."""
    class_id = torch.tensor(table, dtype=torch.uint8, device=DEV)
    priority = torch.ops.mdt.mol_rank(*graph)
    want_p = [priority_of(n, atoms, nb, bonds, width) for n, atoms, nb, bonds in rows]
    torch.cuda.synchronize()
    assert priority.dtype == torch.int64 and [[int(x) & MASK64 for x in row] for row in priority.tolist()] == want_p, what
    kept = None
    for invariant in invariants:
        widest = [W.write_arrays(n, atoms, nb, bonds, p if invariant else None, table, 128, width) for (n, atoms, nb, bonds), p in zip(rows, want_p)]
        for W_ in widths:
            want = [W.at_width(r, W_) for r in widest]
            got = torch.ops.mdt.mol_write(*graph, priority if invariant else None, class_id, W_)
            torch.cuda.synchronize()
            assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.uint8, torch.uint8]
            assert got[3].tolist() == [r["flags"] for r in want] and got[1].tolist() == [r["length"] for r in want], (what, W_, invariant)
            assert got[0].tolist() == [r["tokens"] for r in want] and got[2].tolist() == [r["token_atom"] for r in want], (what, W_, invariant)
            kept = kept or want
    return kept


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("source", ["molecule", 0, 1, 2, 3])
def test_the_whole_pool(source, normalize, pool, vocab):
    """As written and as normal forms; the molecule itself and its scaffold arrays in all four modes; W = 64 and 128; with the
    priority and as numbered."""
    graph = graph_of(pool, vocab, 64, normalize)
    if source == "molecule":
        rows = [C.input_arrays(s, normalize) for s in pool]
    else:
        graph = torch.ops.mdt.mol_scaffold(*graph, source)[:4]
        rows = []
        for s in pool:
            r = C.string_scaffold(s, source, normalize)
            rows.append((r["n"], ) + (C.unpacked(r)[0], r["nb"], C.unpacked(r)[1]))
    want = agree(graph, rows, table_of(vocab), 64, (source, normalize))
    flags = [r["flags"] for r in want]
    print("%s normalize %s: written %d, too long %d, not writable %d, no molecule %d" % (source, normalize, flags.count(1), flags.count(2),
                                                                                        flags.count(8), flags.count(0)))
    assert flags.count(1) >= (1000 if source in ("molecule", 0, 1) else 800) and flags.count(0) >= 6 and flags.count(4) == 0
    if normalize and source == "molecule":
        assert flags.count(2) >= 100                                         # every atom in brackets: rows that need more than 64 tokens


def test_written_rows_read_back_to_the_same_key_and_spellings_to_one_row(spelled, pool, vocab):
    """On the device: mdt::mol_key of mdt::mol_graph of the written rows is mdt::mol_key of the input for every written row that reads
    back with status 0, and the four spellings of each of the 500 graphs give one token row."""
    graph = graph_of(pool, vocab, 64)
    class_id = vocab.class_id_on(DEV)
    key = torch.ops.mdt.mol_key(*graph)
    for invariant in (True, False):
        tokens, length, _, flags = torch.ops.mdt.mol_write(*graph, torch.ops.mdt.mol_rank(*graph) if invariant else None, class_id, 64)
        packed, n, _, _ = torch.ops.mdt.tokens_compact(tokens, 0, 1.0)
        assert torch.equal(packed, tokens) and torch.equal(n, length * (flags == 1))       # written rows are compact
        *again, status, _ = torch.ops.mdt.mol_graph(packed, n, *vocab.on(DEV))
        key_again = torch.ops.mdt.mol_key(*again)
        torch.cuda.synchronize()
        good = (flags == 1) & (status == 0)
        assert int(good.sum()) >= 2000 and int(((flags == 1) & (status != 0)).sum()) == 0
        assert torch.equal(key_again[good], key[good]) and bool((key[good] != 0).all())
        if invariant:
            rows = tokens[:2000].view(500, 4, 64)
            assert bool((flags[:2000] == 1).all()) and bool((rows == rows[:, :1]).all())
        else:
            rows = tokens[:2000].view(500, 4, 64)
            assert int((rows == rows[:, :1]).all(dim=2).all(dim=1).sum()) == 69


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK + 1, 67])
@pytest.mark.parametrize("L", [1, 2, 5, 32, 64])
def test_row_shapes(L, R_, pool, vocab):
    """Molecule rows interleaved with empty rows and rows of status != 0, cut to the width (some become no molecule: a case);
    R is no multiple of the four rows of a workgroup; W = 1, T - 1, T (of the longest written row) and 128."""
    rng = np.random.default_rng(100 * L + R_)
    small = {1: ["c", "C", "*", "", "(", "N", "F", "O"], 2: ["CC", "C=", "cc", "C", "", "C1", "N#", "OO"],
             5: ["C1CC1", "C1CO1", "CC=O", "C1CC", "", "C(C)C", "c1cc1", "C1OC1"]}
    if L in small:
        strings = [small[L][int(rng.integers(8))] for _ in range(R_)]
    else:
        strings = [["", "C(", pool[int(rng.integers(len(pool)))][:L]][min(int(rng.integers(6)), 2)] for _ in range(R_)]
    table = table_of(vocab)
    rows = [C.input_arrays(s, False, L) for s in strings]
    T = max([W.write_arrays(*r, priority_of(*r, L), table, 128, L)["length"] for r in rows] + [2])
    agree(graph_of(strings, vocab, L), rows, table, L, (L, R_), widths=sorted({1, T - 1, T, 128}))
    if L >= 5:
        rows = [C.input_arrays(s, True, L) for s in strings]
        agree(graph_of(strings, vocab, L, True), rows, table, L, (L, R_, "normal form"), widths=(T, 128), invariants=(True,))


def test_no_rows_launches_nothing(vocab):
    n, rows = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV)
    assert tuple(torch.ops.mdt.mol_rank(n, rows, n, rows).shape) == (0, 8)
    out = torch.ops.mdt.mol_write(n, rows, n, rows, None, vocab.class_id_on(DEV), 20)
    assert [tuple(t.shape) for t in out] == [(0, 20), (0,), (0, 20), (0,)]
    empty = torch.zeros(0, 8, dtype=torch.long)
    assert mol_respell(empty, vocab, DEV)[0].shape == (0, 8) and scaffold_tokens(empty, vocab, DEV, width=5)[0].shape == (0, 5)
    assert scaffold_keep(empty, vocab, DEV)[1].shape == (0, 8) and mol_write(n, rows, n, rows, vocab, DEV, width=3)[0].shape == (0, 3)


def test_graph_arrays_that_no_scan_writes(vocab):
    """The %10 ladder, each reason not to write, the longest atom text on 64 atoms, the arrays of the scaffold test (a ring of all 64
    lanes, entries listed twice, entries (x, x), counts outside the row, the complete graph on 8 atoms) -- under the full
    vocabulary, and under vocabularies without '%', without '[' and without '(', '=' and '1'."""
    special = W.special_rows()
    full = dict(W.ASCII)
    tables = [W.class_table(full)] + [W.class_table({i: ch for i, ch in full.items() if ch not in gone}) for gone in ("%", "[", "(=1")]
    for width in sorted({row[0] for row in special}):
        rows = [(n, atoms, nb, bonds) for w, n, nb, atoms, bonds in special if w == width]
        graph = device_arrays(rows, width)
        for v, table in enumerate(tables):
            want = agree(graph, rows, table, width, (width, v), widths=(47, 128) if v == 0 else (128,), invariants=(False, True) if v == 0 else (False,))
            if width == 64 and v == 0:
                ladder = want[[row[1:] for row in special if row[0] == 64].index(W.ladder()[1:])]        # (as numbered, W = 47)
                text = "".join(chr(t) for t in ladder["tokens"][:ladder["length"]])
                assert ladder["flags"] == 1 and text.count("%10") == 2 and ladder["length"] == 46
    flags = [W.write_arrays(n, atoms, nb, bonds, None, tables[0], 128, w)["flags"] for w, n, nb, atoms, bonds in special]
    assert flags.count(8) >= 9 and flags.count(0) >= 5 and flags.count(1) >= 5 and flags.count(2) >= 1


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry points on outputs pre-filled by poison_util (NaN bits, then large garbage), each followed by a guard band of the same
    fill: every output word comes out defined, zero beyond the length and beyond natoms, and the guard comes back as it was."""
    strings = pool[::9] + NO_MOLECULE + LONG
    table = table_of(vocab)
    class_id = vocab.class_id_on(DEV)
    for L, W_, fill, invariant in ((64, 64, P.NAN, True), (37, 128, P.GARBAGE, False), (37, 29, P.NAN, True)):
        rows = [s[:L] for s in strings]
        inputs = graph_of(rows, vocab, L)
        R_ = len(rows)
        guard = 64                                                           # words of the fill after each output
        sizes = [(2 * R_ * L, torch.int64, (R_, L)), (R_ * W_, torch.int32, (R_, W_)), (R_, torch.int32, (R_,)), (R_ * W_, torch.uint8, (R_, W_)),
                 (R_, torch.uint8, (R_,))]
        raw, out, before = [], [], []
        for seed, (count, dtype, shape) in enumerate(sizes):
            words = (count + 3) // 4 if dtype == torch.uint8 else count
            image = P.fill_bits(fill, words + guard, seed, DEV)
            raw.append(image)
            before.append(image.clone())
            cut = image[:words].view(dtype) if dtype != torch.uint8 else image.view(torch.uint8)[:count]
            out.append(cut.view(shape))
        lib = rt.load_library()
        with torch.cuda.device(DEV):
            rt.check(lib.mdt_mol_rank(*[rt.ptr(t) for t in inputs], L, R_, rt.ptr(out[0]), rt.current_stream()))
            rt.check(lib.mdt_mol_write(*[rt.ptr(t) for t in inputs], rt.ptr(out[0]) if invariant else 0, L, R_, rt.ptr(class_id), W_,
                                       *[rt.ptr(t) for t in out[1:]], rt.current_stream()))
        torch.cuda.synchronize()
        graphs = [C.input_arrays(s, False, L) for s in rows]
        want_p = [priority_of(*g, L) for g in graphs]
        want = [W.write_arrays(*g, p if invariant else None, table, W_, L) for g, p in zip(graphs, want_p)]
        assert [[int(x) & MASK64 for x in row] for row in out[0].tolist()] == want_p, L
        assert out[1].tolist() == [r["tokens"] for r in want] and out[2].tolist() == [r["length"] for r in want], L
        assert out[3].tolist() == [r["token_atom"] for r in want] and out[4].tolist() == [r["flags"] for r in want], L
        assert sum(r["flags"] == 1 for r in want) > 50 and sum(r["flags"] == 0 for r in want) >= 6
        beyond = torch.arange(W_, device=DEV).unsqueeze(0) >= (out[2] * (out[4] == 1)).long().unsqueeze(1)
        assert not out[1][beyond].any() and not out[3][beyond].any()
        beyond_atoms = torch.arange(L, device=DEV).unsqueeze(0) >= inputs[0].long().unsqueeze(1)
        assert not out[0][beyond_atoms].any()
        for image, was, (count, dtype, _) in zip(raw, before, sizes):        # what lies after the outputs is nobody's
            nbytes = count * (1 if dtype == torch.uint8 else 4)
            assert torch.equal(image.view(torch.uint8)[nbytes:], was.view(torch.uint8)[nbytes:])


def test_the_public_calls(pool, vocab):
    rows = pool[::5] + list(C.TABLE) + NO_MOLECULE + LONG
    ids = vocab.encode(rows, 64)
    table = table_of(vocab)
    status = [S.check(s)[0] for s in rows]
    for normalize, invariant, width in ((False, True, None), (True, True, 128), (False, False, 40)):
        W_ = width or 64
        graphs = [C.input_arrays(s, normalize) for s in rows]
        want = [W.write_arrays(*g, priority_of(*g, 64) if invariant else None, table, W_) for g in graphs]
        tokens, flags, st, position = mol_respell(ids.to(torch.int16), vocab, DEV, normalize=normalize, invariant=invariant, width=width)
        arrays = [torch.tensor(x) for x in ([g[0] for g in graphs], [list(g[1]) + [0] * (64 - g[0]) for g in graphs], [g[2] for g in graphs],
                                            [[N.pack(e) for e in g[3]] + [0] * (64 - g[2]) for g in graphs])]
        direct = mol_write(*arrays, vocab, DEV, width=W_, invariant=invariant)
        torch.cuda.synchronize()
        assert all(t.dtype == torch.int64 for t in (tokens, flags, st, position) + direct)
        assert tokens.tolist() == [r["tokens"] for r in want] == direct[0].tolist() and flags.tolist() == [r["flags"] for r in want] == direct[3].tolist()
        assert direct[1].tolist() == [r["length"] for r in want] and direct[2].tolist() == [r["token_atom"] for r in want]
        assert st.tolist() == status and vocab.decode(tokens) == [r["text"] if r["flags"] == 1 else "" for r in want]
    for kw, mode, normalize in ((dict(), 1, False), (dict(exocyclic=False, normalize=True, width=128), 0, True), (dict(generic=True, width=50), 3, False)):
        W_ = kw.get("width", 64)
        scaffolds = [C.string_scaffold(s, mode, normalize) for s in rows]
        want = [W.graph_write(*C.unpacked(r), table, W_) for r in scaffolds]
        tokens, flags, scaffold_flags, st, position = scaffold_tokens(ids, vocab, DEV, **kw)
        torch.cuda.synchronize()
        assert tokens.tolist() == [r["tokens"] for r in want] and flags.tolist() == [r["flags"] for r in want], kw
        assert scaffold_flags.tolist() == [r["flags"] for r in scaffolds] and st.tolist() == status
    by = dict(zip(rows, vocab.decode(scaffold_tokens(ids, vocab, DEV)[0])))
    assert by["Cc1ccccc1"] == by["CC(=O)c1ccccc1"] == W.respell("c1ccccc1") == "c1ccccc1" and by["CCO"] == "" and by["O=C1CCCCC1"] == "C1CCCCC1=O"
    for kw, mode, normalize in ((dict(), 1, False), (dict(exocyclic=False, normalize=True, width=128), 0, True)):
        W_ = kw.get("width", 64)
        tokens, keep, flags, st, position = scaffold_keep(ids, vocab, DEV, **kw)
        torch.cuda.synchronize()
        graphs = [C.input_arrays(s, normalize) for s in rows]
        want = [W.write_arrays(*g, priority_of(*g, 64), table, W_) for g in graphs]
        maps = [C.string_scaffold(s, mode, normalize)["atom_map"] for s in rows]
        mask = [[o != 0 and m[o - 1] != 0 for o in r["token_atom"]] for r, m in zip(want, maps)]
        assert keep.dtype == torch.bool and keep.tolist() == mask and tokens.tolist() == [r["tokens"] for r in want], kw
        assert flags.tolist() == [r["flags"] for r in want] and st.tolist() == status
        assert sum(any(m) for m in mask) >= 100 and sum(r["flags"] == 1 and not any(m) for r, m in zip(want, mask)) >= 50


def test_refining_a_lead_around_its_scaffold():
    """scaffold_keep()'s mask fed to refine_keep_tokens() on the tiny model: every kept position of the output is the written row's
    token -- refine_keep_tokens()'s own guarantee, now reachable from a molecule."""
    m = make_model("tiny")                                                   # 16 ids, rows of 32 positions
    vocab = SmilesVocabulary([None] + list("CNOcno1()-=#[H]"))
    leads = ["Cc1ccccc1", "CC(=O)c1ccccc1", "OCC", "NC1CC1C(=O)O", "c1cc[nH]c1", "C(", "O=C1CCC1CN"]
    assert len(vocab) == 15 == m.pred_dim - 1 and m.max_length == 32
    tokens, keep, flags, status, _ = scaffold_keep(vocab.encode(leads, 32), vocab, DEV)
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 1, 1, 1, 1, 0, 1] and keep.sum(dim=1).tolist()[:3] == [10, 10, 0] and not keep[5].any()
    assert vocab.decode(tokens)[:3] == ["c1ccc(cc1)C", "c1c(cccc1)C(=O)C", "OCC"]
    B, T = len(leads), 8                                                    # (a start step is at most T - 2)
    seq = synth_normal("molwrite/seq", (B, 12))
    for start in (2, [0, 5, 3, 1, 4, 2, 6]):
        out = m.refine_keep_tokens(seq, DEV, tokens.cpu(), start_step=start, cond_scale=2.0, timesteps=T, noise=NoiseSource(seed=17),
                                   keep_mask=keep.cpu())
        torch.cuda.synchronize()
        assert out.shape == tokens.shape and torch.equal(out[keep], tokens[keep]) and int(keep.sum()) >= 40
