"""The loader schedule of csrc/mdt_ring_sched.h ("half a tile further ahead", k_tf256.hip) replayed on the host by
tools/ring_sched_check.cpp: no piece is issued into bytes a compute wave may still read, every byte a unit reads is covered by
the counted wait of its publishing barrier, every tile is issued exactly once -- over the descriptor tables of the compiled
programs and over hand-made streams for every neighbourhood of tile kinds.  Host code only: built with the host compiler, and
once more with AddressSanitizer and UBSan."""
import itertools
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
P, O, K, V, SCR, SCRV = range(6)
NAMES = "POKVSs"


def _cxx():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return c
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("ring_sched")
    out = {}
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(d / f"ring_sched_check_{name}")
        subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tools", "ring_sched_check.cpp"), "-o", exe],
                       check=True, capture_output=True, text=True)
        out[name] = exe
    return out


def _write(path, recs):
    with open(path, "w") as f:
        for name, f32, npw, words in recs:
            f.write(f"S {name} {f32} {npw} {len(words)}\n" + " ".join(str(w) for w in words) + "\n")


def _stream(kinds):
    """Descriptor words of a list of kinds: weight tiles count up through the pool, K / V carry (layer, head), the vector
    descriptor an (offset, parity) word -- the checker reads the kinds, the words only have to be well-formed."""
    return [k | (n << 3) for n, k in enumerate(kinds)]


def _run(exe, path, *args):
    r = subprocess.run([exe, *args, path], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def test_compiled_programs(checkers, tmp_path):
    """Every MDT_OP_TF256 descriptor table of cfg1 (narrow, wide, the dual-batch guidance program), sparse and cfg3, split-bf16
    and fp32 tiles."""
    import ring_sched_dump
    recs = ring_sched_dump.records()
    names = [r[0] for r in recs]
    for need in ("cfg1.bf16x3.narrow.eval.", "cfg1.bf16x3.wide.eval.", "cfg1.bf16x3.narrow.eval_dual.", "cfg1.f32.narrow.eval.", "sparse."):
        assert any(n.startswith(need) for n in names), need
    assert any(r[2] == 6 for r in recs) and any(r[2] == 0 for r in recs)       # with and without cross-attention
    path = str(tmp_path / "streams.txt")
    _write(path, recs)
    for which in ("plain", "san"):
        rc, out = _run(checkers[which], path)
        assert rc == 0, out
        assert f"{len(recs)} streams" in out and " 0 violations" in out
    # the headline kernel's streams do use the schedule (some tiles ARE issued half a tile ahead), and the check bites: with a
    # split-bf16 P tile wrongly taken to have a dead half the same streams violate (a)
    assert " 0 issued half a tile ahead" not in out
    rc, out = _run(checkers["plain"], path, "--assume-p-dead")
    assert rc == 1 and "(a) piece issued into bytes still in use" in out


NAMED = {                       # the neighbourhoods the loader meets, in a stream long enough for every slot to be reused
    "P_P": [P] * 12,
    "P_O": [P, P, O, O] * 3,
    "O_K": [P, P, O, O, K, V, O, O, P, P, K, V],
    "K_V": [P, P, K, V, O, O] * 2,
    "V_O": [P, P, K, V, O, O, O, O, K, V, O, O],
    "self_attention": [P] * 6 + [O] * 2 + [P] * 6 + [O] * 2,
    "scratch_between": [P, P, O, O, SCRV, SCR, P, P, O, O, SCR, SCR],
    "pair_scratch": [P, P, O, O, SCRV, SCR, SCR, SCR, P, P, O, O, SCR, SCR, SCR, SCR],
    "O_scratch_K": [O, O, O, O, SCRV, SCR, K, V, O, O, SCR, SCR],
    "one_tile": [P],
    "one_scratch": [SCR],
    "two_tiles": [P, O],
    "three_tiles": [O, O, P],
    "four_tiles": [O, O, O, O],
    "five_tiles": [O, O, O, O, O],
    "ends_split": [O] * 9,                   # the last tile of the launch is itself issued in two halves
}


def test_hand_made_neighbourhoods(checkers, tmp_path):
    """Named streams, then EVERY window of five consecutive tile kinds (what a tile's schedule depends on: its own kind, the
    kind four tiles back whose slot it takes, and what is issued around it) between two paddings, for both product types and
    K / V tiles of 1, 3 and 6 pieces."""
    recs = []
    for name, kinds in NAMED.items():
        for f32 in (0, 1):
            recs.append((f"{name}.{'f32' if f32 else 'bf16'}", f32, 6, _stream(kinds)))
    pads = ([P, O, P, O, O], [O] * 5)
    for n, win in enumerate(itertools.product(range(6), repeat=5)):
        pad = pads[n % 2]
        name = "w_" + "".join(NAMES[k] for k in win)
        recs.append((name + ".bf16", 0, (1, 3, 6)[n % 3], _stream(pad + list(win) + pad)))
        recs.append((name + ".f32", 1, (6, 1, 3)[n % 3], _stream(pad + list(win) + pad)))
    path = str(tmp_path / "hand.txt")
    _write(path, recs)
    for which in ("plain", "san"):
        rc, out = _run(checkers[which], path)
        assert rc == 0, out
        assert f"{len(recs)} streams" in out and " 0 violations" in out


def test_header_constants():
    """The clean halves the header derives (static_asserts in mdt_ring_sched.h) are the ones the kernel's dispatch names: a
    host compile of the header alone is enough to evaluate them."""
    src = ('#include "mdt_ring_sched.h"\nusing namespace mdt::ring;\n'
           "static_assert(early_mask(false, 8, T_P, T_O) == 0x33 && early_mask(false, 8, T_O, T_P) == 0, \"bf16\");\n"
           "static_assert(early_mask(true, 8, T_O, T_P) == 0x55 && early_mask(true, 8, T_P, T_O) == 0x0f, \"f32\");\n"
           "static_assert(early_mask(true, 3, T_P, T_P) == 0 && early_mask(true, 8, T_K, T_P) == 0 && early_mask(true, 8, T_P, T_V) == 0 &&\n"
           "              early_mask(true, 8, T_P, T_SCRATCH) == 0 && early_mask(true, 8, T_SCRATCH_VEC, T_P) == 0, \"whole\");\n"
           "int main() { Allowance a; a.prev_total = 8; a.turn(4, 4, 1); a.turn(8, 0, 0); return a.at_barrier() == 13 ? 0 : 1; }\n")
    r = subprocess.run([_cxx(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc"),
                        "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
