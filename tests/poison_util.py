"""Poisoning harness: results must not depend on memory that no operand owns.

The CPU interpreter (oracle/program_interp.py) touches every operand through Buffers.view().  TracingBuffers records those
ranges; their union is the OWNED SET of a program, everything else in a buffer is NOBODY'S.  check_poisoned() runs a program
with nobody's floats -- and a guard band on either side of every buffer -- holding zeros, then a NaN pattern, then large finite
garbage, and asserts bit for bit that the owned floats do not change with the fill and that nobody's floats come back untouched.
No GPU code of its own: the caller hands in the function that runs the ops (the C-ABI runner below, or an interpreter-based one).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from moleculediffusiontransformer_amd import runtime as rt
from oracle.program_interp import Buffers, run_program

GUARD = 65536                  # floats on each side of every buffer: one 64-row tile of the widest (1024-float) row
ZERO, NAN, GARBAGE = "ZERO", "NAN", "GARBAGE"
# a NaN as fp32 AND as each of its two bf16 halves (0x7FC00000 has a zero bf16 half: a kernel reading bf16 would see 0.0)
NAN_BITS = 0x7FC17FC1


def fill_bits(fill: str, n: int, seed: int = 0, device="cpu") -> torch.Tensor:
    """n int32 words of a fill, made on `device`.  GARBAGE: seeded, finite, magnitudes 1e3 .. 1e4, random signs -- built as PAIRS
    of such bf16 values, so the word is in that range as fp32 (the high half with 16 more mantissa bits) and as either bf16 half.
    It catches what a NaN cannot: fmaxf, v_med3 and comparisons swallow a NaN but take a large finite value."""
    if fill == ZERO:
        return torch.zeros(n, dtype=torch.int32, device=device)
    if fill == NAN:
        return torch.full((n,), NAN_BITS, dtype=torch.int32, device=device)
    assert fill == GARBAGE, fill
    g = torch.Generator(device=device).manual_seed(0x5EED + seed)
    mag = 10.0 ** (3.0 + torch.rand(2 * n, generator=g, device=device))
    sign = torch.randint(0, 2, (2 * n,), generator=g, device=device).float() * 2.0 - 1.0
    halves = (mag * sign).clamp(-9984.0, 9984.0).to(torch.bfloat16)
    return halves.view(torch.int32).clone()


def fill_floats(fill: str, n: int, seed: int = 0, device="cpu") -> torch.Tensor:
    return fill_bits(fill, n, seed, device).view(torch.float32)


def poison_(t: torch.Tensor, fill: str, seed: int = 0) -> None:
    """Overwrites every 4-byte word of tensor `t` with the fill (made on the tensor's device)."""
    assert t.element_size() == 4 and t.is_contiguous()
    if t.numel():
        t.view(-1).view(torch.int32).copy_(fill_bits(fill, t.numel(), seed, t.device))


class TracingBuffers(Buffers):
    """Buffers that remember every [off, off + n) the interpreter views, per space ('weights', 'act', 'shr', ('ext', slot));
    act offsets scaled by B, as view() does.  `op_index` (set by trace_program) tags each range with the op that touched it."""

    def __init__(self, weights, act, shr, ext):
        super().__init__(weights, act, shr, ext)
        self.ranges: Dict[object, List[Tuple[int, int, int]]] = {}
        self.op_index = -1

    def view(self, ref, B: int, n: int) -> Optional[torch.Tensor]:
        if ref.space == rt.SP_WEIGHT:
            key, off = "weights", ref.off
        elif ref.space == rt.SP_ACT:
            key, off = "act", ref.off * B
        elif ref.space == rt.SP_SHR:
            key, off = "shr", ref.off
        elif ref.space != rt.SP_NONE:
            key, off = ("ext", ref.space - rt.SP_EXT0), ref.off
        if ref.space != rt.SP_NONE:
            self.ranges.setdefault(key, []).append((int(off), int(off) + int(n), self.op_index))
        return super().view(ref, B, n)

    def _buf(self, key):
        return self.ext[key[1]] if isinstance(key, tuple) else getattr(self, key)

    def owned(self, key) -> torch.Tensor:
        """bool mask over the buffer: True = inside the footprint of some op."""
        m = torch.zeros(self._buf(key).numel(), dtype=torch.bool)
        for lo, hi, _ in self.ranges.get(key, ()):
            m[lo:hi] = True
        return m

    def ops_at(self, key, off: int) -> List[int]:
        return sorted({k for lo, hi, k in self.ranges.get(key, ()) if lo <= off < hi})


def trace_program(ops, bufs: TracingBuffers, B: int, n_shr: int = 0) -> None:
    """run_program op by op (it is a plain loop over the ops), tagging the ranges of each."""
    for k, op in enumerate(ops):
        bufs.op_index = k
        run_program([op], bufs, B, n_shr)
    bufs.op_index = -1


def interp_run(ops, weights, act, shr, ext, B, n_shr=0) -> None:
    """The honest CPU runner: the interpreter on the buffers it is given."""
    run_program(ops, Buffers(weights, act, shr, ext), B, n_shr)


def gpu_run(ops, weights, act, shr, ext, B, n_shr=0) -> None:
    """The C-ABI runner of gpu_util.run_both, on device buffers it is given."""
    b = rt.MdtBindings()
    b.weights, b.act, b.shr = rt.ptr(weights), rt.ptr(act), rt.ptr(shr)
    for k, v in ext.items():
        b.ext[k] = rt.ptr(v)
    with torch.cuda.device(weights.device):
        rt.Program(ops).run(b, B, n_shr)
        torch.cuda.synchronize()


def _op_names(ops, idx=None) -> str:
    ks = range(len(ops)) if idx is None else idx
    return ", ".join(f"#{k} {rt.OP_NAMES.get(ops[k].kind, ops[k].kind)}" for k in ks) or "no op"


def _first(mask: torch.Tensor) -> int:
    return int(mask.nonzero()[0])


def check_poisoned(run: Callable, ops, weights, act, shr, ext, B, n_shr=0, *, fills=(NAN, GARBAGE), device="cpu"):
    """Runs `ops` through `run(ops, weights, act, shr, ext, B, n_shr)` (in place on the buffers it is handed, on `device`) with
    zeros and then each of `fills` in every float no operand owns and in GUARD floats either side of every buffer; asserts the
    contract (module docstring).  Returns ((act, shr, ext) of the baseline run on the CPU, (act, shr, ext) of the interpreter) --
    the shape gpu_util.run_both returns, so it can stand in for it."""
    ext = {k: v.contiguous().view(-1) for k, v in ext.items()}
    for t in (weights, act, shr, *ext.values()):
        assert t.element_size() == 4, "the harness handles 4-byte elements"
    # 1. owned set + CPU result
    cpu = TracingBuffers(weights.clone(), act.clone(), shr.clone(), {k: v.clone() for k, v in ext.items()})
    trace_program(ops, cpu, B, n_shr)
    keys = ["weights", "act", "shr"] + [("ext", k) for k in ext]
    given = {"weights": weights, "act": act, "shr": shr, **{("ext", k): v for k, v in ext.items()}}
    orig = {k: given[k].contiguous().view(-1).view(torch.int32) for k in keys}
    viewed = {k: k in cpu.ranges or not isinstance(k, tuple) for k in keys}      # ext the interpreter never views: guards only
    owned = {k: (cpu.owned(k) if viewed[k] else torch.ones(orig[k].numel(), dtype=torch.bool)) for k in keys}
    name = lambda k: k if isinstance(k, str) else f"ext[{k[1]}]"      # noqa: E731

    def image(k, fill, seed):
        """[guard | buffer | guard] as int32: the fill in the guards and on nobody's floats, the caller's values on the owned set
        (ZERO: the caller's values on the whole buffer -- the baseline is the run the suite has always made)."""
        n = orig[k].numel()
        img = fill_bits(fill, n + 2 * GUARD, seed)
        inner = img[GUARD: GUARD + n]
        if fill == ZERO:
            inner.copy_(orig[k])
        else:
            inner[owned[k]] = orig[k][owned[k]]
        return img

    def once(fill):
        imgs = {k: image(k, fill, s) for s, k in enumerate(keys)}
        dev = {k: v.clone().to(device) for k, v in imgs.items()}
        inner = {k: dev[k][GUARD: GUARD + orig[k].numel()].view(torch.float32) for k in keys}
        run(ops, inner["weights"], inner["act"], inner["shr"], {k[1]: inner[k] for k in keys if isinstance(k, tuple)}, B, n_shr)
        return imgs, {k: v.cpu() for k, v in dev.items()}

    # 2. / 3. baseline, twice: a program that is not repeatable cannot be compared across fills
    _, base = once(ZERO)
    _, again = once(ZERO)
    for k in keys:
        if not torch.equal(base[k], again[k]):
            off = _first(base[k] != again[k]) - GUARD
            raise AssertionError(f"not repeatable: {name(k)}[{off}] differs between two runs on identical buffers "
                                 f"({_op_names(ops, cpu.ops_at(k, off) or None)})")
    # 4. / 5. the poisoned runs
    for fill in fills:
        before, after = once(fill)
        for k in keys:
            n = orig[k].numel()
            own = torch.zeros(n + 2 * GUARD, dtype=torch.bool)
            own[GUARD: GUARD + n] = owned[k]
            # (b) nobody's floats and the guards come back bit for bit
            moved = (after[k] != before[k]) & ~own
            if moved.any():
                off = _first(moved) - GUARD
                where = "guard band" if off < 0 or off >= n else "a float no operand owns"
                raise AssertionError(f"wrote memory no operand owns under {fill}: {name(k)}[{off}] ({where}) changed "
                                     f"({_op_names(ops)})")
            # (a) every owned float equals the baseline
            diff = (after[k] != base[k]) & own
            if diff.any():
                off = _first(diff) - GUARD
                a, b_ = after[k].view(torch.float32)[off + GUARD].item(), base[k].view(torch.float32)[off + GUARD].item()
                raise AssertionError(f"depends on memory no operand owns under {fill}: {name(k)}[{off}] = {a!r}, baseline {b_!r}; "
                                     f"{int(diff.sum())} floats differ ({_op_names(ops, cpu.ops_at(k, off) or None)})")
            # (c) finite wherever the baseline is (implied by (a); kept as its own statement)
            bad = own & torch.isfinite(base[k].view(torch.float32)) & ~torch.isfinite(after[k].view(torch.float32))
            assert not bad.any(), f"non-finite output under {fill}: {name(k)}[{_first(bad) - GUARD}] ({_op_names(ops)})"

    def inner_f32(k):
        return base[k][GUARD: GUARD + orig[k].numel()].clone().view(torch.float32)
    return ((inner_f32("act"), inner_f32("shr"), {k: inner_f32(("ext", k)) for k in ext}), (cpu.act, cpu.shr, cpu.ext))
