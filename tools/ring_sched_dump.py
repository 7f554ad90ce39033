#!/usr/bin/env python3
"""Writes the tile descriptor tables of every MDT_OP_TF256 op of the compiled programs (cfg1 narrow and wide, its dual-batch guidance
program, sparse, cfg3; split-bf16 and fp32 tiles) as input of tools/ring_sched_check.cpp -- no GPU, no library:

    python tools/ring_sched_dump.py streams.txt [case ...]

Per table one record "S name f32 npw NT" and the NT words (kind | aux << 3); npw = LDS-DMA pieces per loader wave of a K / V tile.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from helpers import CASES, synth_sd  # noqa: E402
from moleculediffusiontransformer_amd import runtime as rt  # noqa: E402
from moleculediffusiontransformer_amd.compiler import compile_unet  # noqa: E402
from moleculediffusiontransformer_amd.netspec import forward_unet_config, inverse_unet_config, sparse_unet_config  # noqa: E402


def tables(op, weights):
    """(half, words) of one MDT_OP_TF256 op."""
    i = op.i
    nt, nsplit = i[rt.F_NT], 2 if i[rt.F_NSPLIT] == 2 else 1
    words = weights[op.p0.off: op.p0.off + nsplit * nt].contiguous().view(torch.int32).tolist()
    return [(hh, words[hh * nt: (hh + 1) * nt]) for hh in range(nsplit)]


def records(cases=("cfg1", "sparse", "cfg3")):
    out = []
    for case in cases:
        kind, kw = CASES[case]
        mk = {"inverse": inverse_unet_config, "forward": forward_unet_config, "sparse": sparse_unet_config}[kind]
        ucfg = mk(kw["pred_dim"], kw["channels"], 128, kw["context_embedding_max_length"])
        usd = {k[5:]: v for k, v in synth_sd(case).items() if k.startswith("unet.")}
        for mode in ("bf16x3", "f32"):
            for wide in (False, True):
                cu = compile_unet(ucfg, kw["max_length"], kw["context_embedding_max_length"], usd, max_time_rows=4, gemm_mode=mode, tf256=wide)
                for pname, prog in sorted(cu.programs.items()):
                    for n, op in enumerate(prog):
                        if op.kind != rt.OP_TF256:
                            continue
                        i = op.i
                        npw = ((32 // i[rt.F_T]) * i[rt.F_TK] + 15) // 16 if i[rt.F_CROSS] else 0
                        for hh, words in tables(op, cu.weights):
                            name = f"{case}.{mode}.{'wide' if wide else 'narrow'}.{pname}.op{n}.half{hh}"
                            out.append((name, int(bool(i[rt.F_WF32])), npw, words))
    return out


def write(path, recs):
    with open(path, "w") as f:
        for name, f32, npw, words in recs:
            f.write(f"S {name} {f32} {npw} {len(words)}\n" + " ".join(str(w & 0xffffffff) for w in words) + "\n")


if __name__ == "__main__":
    recs = records(tuple(sys.argv[2:]) or ("cfg1", "sparse", "cfg3"))
    write(sys.argv[1], recs)
    print(f"{len(recs)} descriptor tables, {sum(len(r[3]) for r in recs)} tiles -> {sys.argv[1]}")
