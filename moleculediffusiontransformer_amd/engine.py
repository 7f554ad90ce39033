"""Device-side state of one compiled U-Net: packed weights, arenas, programs, HIP-graph replay.

PyTorch supplies device memory and the current HIP stream only; all arithmetic is in
libmdt_hip.so (see include/mdt_hip.h).  There is no CPU path: constructing an engine on a
machine without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch

from . import runtime as rt
from .compiler import EXT_CTX, EXT_FILM, EXT_OUT, EXT_XBUF, EXT_XFLAGS, EXT_XIN, CompiledUNet


def _require_gpu(device: torch.device) -> None:
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(
            "moleculediffusiontransformer_amd runs its sampling path only on an AMD GPU through libmdt_hip.so; "
            f"device '{device}' is not a HIP device (there is no CPU fallback by design)")


class UNetEngine:
    """Runs the `time`, `ctx`, `eval` and `eval_fixed` programs of a CompiledUNet for a batch -- or, for the per-row form
    (CompiledUNet.rows: one noise level per sample), `time_rows`, `ctx`, `eval_rows` and `eval_rows_fixed`."""

    def __init__(self, compiled: CompiledUNet, device, use_graph: Optional[bool] = None):
        device = torch.device(device)
        _require_gpu(device)
        rt.load_library()
        self.c = compiled
        self.device = device
        with torch.cuda.device(device):
            self.weights = compiled.weights.to(device)
            self.shr = torch.zeros(compiled.shr_floats, device=device)
            try:
                self.programs: Dict[str, rt.Program] = {k: rt.Program(v) for k, v in compiled.programs.items()}
            except RuntimeError as e:
                if "mdt_program_create" not in str(e):      # only validation errors mean "outside the envelope"
                    raise
                raise RuntimeError(
                    f"U-Net configuration outside the envelope of the MI355X kernels (max_length={compiled.length}, "
                    f"channels={compiled.cfg.channels}, patch_size={compiled.cfg.patch_size}): {e}.  Supported: at most 8192 "
                    "tokens per sample on an attention level, head_features 64, channels a multiple of 16 -- see DESIGN.md "
                    "section 8") from e
            tile = compiled.length * (compiled.in_pad + 1) * 4
            if tile > 160 * 1024:
                raise RuntimeError(f"max_length={compiled.length} with {compiled.in_pad} (padded) channels needs a {tile}-byte "
                                   "sampler tile; the preconditioning / update kernels stage one sample in the 160 KiB of LDS of a "
                                   "compute unit (max_length * (pred_dim_padded + 1) * 4 <= 163840) -- see DESIGN.md section 8")
        if use_graph is None:
            use_graph = os.environ.get("MDT_GRAPH", "1") != "0"
        self.use_graph = use_graph
        self.B = 0
        self.act = None
        self.xin = None           # (B, L, Cp) token-major U-Net input
        self.pred = None          # (B, L, Cp) token-major U-Net output
        self.pred_fixed = None
        self.xflags = self.xbuf = None
        self.film = None          # per-row form: (B, ss_total) per-sample (scale | shift) rows
        self._graphs: Dict[str, torch.cuda.CUDAGraph] = {}
        self._time_rows = 0
        self._fixed_ready = False

    # ------------------------------------------------------------------ buffers
    def reserve(self, B: int) -> None:
        """(Re)allocate per-batch buffers.  Invalidates captured graphs when B changes.  `act`, `film` and `xbuf` come from
        torch.empty and arena slots are reused: callers and kernels must not assume anything about their contents."""
        if B == self.B:
            return
        c = self.c
        self._graphs.clear()
        self.act = self.xin = self.pred = self.pred_fixed = None
        self.act = torch.empty(c.act_floats * B, device=self.device)
        self.xin = torch.zeros(B, c.length, c.in_pad, device=self.device)
        self.pred = torch.zeros(B, c.length, c.in_pad, device=self.device)
        self.pred_fixed = torch.zeros(B, c.length, c.in_pad, device=self.device)
        self.xflags = self.xbuf = None
        self.film = torch.empty(B, c.ss_total, device=self.device) if c.rows else None
        if c.xchg_tokens:
            # pair-split MDT_OP_TF256 (k_tf256.hip): per 32-row block two hand-off blocks of 32 x 256 fp32 in two parities, and
            # one 128-byte flag line per (row block, half) behind 64 diagnostic words.  The flags count hand-offs monotonically
            # over the life of the buffer: zeroed here, never between launches.
            nrb = (B * c.xchg_tokens + 31) // 32
            self.xflags = torch.zeros(64 + 64 * nrb + (8 * 4096 + 16384 if os.environ.get("MDT_XH_LOG") else 0), dtype=torch.int32,
                                      device=self.device)
            self.xbuf = torch.empty(2 * nrb * 2 * 32 * 256, device=self.device)
        self.B = B

    def _bind(self, xin=None, ctx=None, out=None) -> rt.MdtBindings:
        b = rt.MdtBindings()
        b.weights, b.act, b.shr = rt.ptr(self.weights), rt.ptr(self.act), rt.ptr(self.shr)
        b.ext[EXT_XIN], b.ext[EXT_CTX], b.ext[EXT_OUT] = rt.ptr(xin), rt.ptr(ctx), rt.ptr(out)
        b.ext[EXT_XFLAGS], b.ext[EXT_XBUF] = rt.ptr(getattr(self, "xflags", None)), rt.ptr(getattr(self, "xbuf", None))
        b.ext[EXT_FILM] = rt.ptr(getattr(self, "film", None))
        return b

    # A pair hand-off that runs into its time-out (a partner workgroup was never scheduled: the two workgroups of a pair must be
    # resident at the same time; launch_tf256 never puts more workgroups into a launch than the device runs at once, but compute
    # units held by another stream or process, or a CU mask, are invisible to it) raises bit 0 of the diagnostic word on the
    # device and the launch's rows are garbage.  Every sampling loop and every net() evaluation copies that word to pinned host
    # memory behind its last launch (note_handoff) and -- by default -- WAITS for the copy and raises before any result is
    # returned (sync_handoff_check: one event wait per call, i.e. ONE HOST SYNCHRONISATION per sample() and per
    # torch.ops.mdt.unet_eval / denoise evaluation; VERDICT r3 #9 / ADVICE r3).  Pipelined callers (user sampler loops built on
    # denoise_fn) defer the look to the next call or to an explicit handoff_check(wait=True) with model.defer_handoff_check;
    # under a stream capture nothing is waited for (see note_handoff).
    sync_handoff_check = True

    def note_handoff(self) -> None:
        if getattr(self, "xflags", None) is None:
            return
        if getattr(self, "_xstat_host", None) is None:
            self._xstat_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._xstat_event = torch.cuda.Event()
        if torch.cuda.is_current_stream_capturing():
            # inside a user's graph capture (torch.ops.mdt.unet_eval in a captured region): a host wait would invalidate the
            # capture, and the copy would be replayed into stale pinned memory.  The status word stays on the device; the next
            # un-captured call -- or handoff_status() -- reports a time-out of the replays.  The capture is REMEMBERED:
            # the next un-captured note_handoff() / handoff_check() says that the word may stem from replays of that graph
            # (without this, the next plain call was blamed for a time-out that happened in a replay).  Sticky: the
            # engine cannot know when that graph is replayed.
            self._xstat_captured = True
            return
        self._xstat_host.copy_(self.xflags[:1], non_blocking=True)
        self._xstat_event.record()
        self._xstat_pending = True
        if self.sync_handoff_check:
            self.handoff_check(wait=True)

    def handoff_check(self, wait: bool = False) -> None:
        """Raises RuntimeError if a call noted by note_handoff() had a hand-off time-out (and clears the word)."""
        if not getattr(self, "_xstat_pending", False):
            if getattr(self, "_xstat_captured", False) and wait and getattr(self, "xflags", None) is not None \
                    and not torch.cuda.is_current_stream_capturing():
                # evaluations were captured into a caller's graph and nothing has looked at the status word since: look now
                self._xstat_host.copy_(self.xflags[:1], non_blocking=True)
                self._xstat_event.record()
                self._xstat_pending = True
            else:
                return
        if wait:
            self._xstat_event.synchronize()
        if not self._xstat_event.query():
            return
        self._xstat_pending = False
        if int(self._xstat_host[0]) != 0:
            if getattr(self, "xflags", None) is not None:
                self.xflags[0] = 0
            when = "this" if wait else "the PREVIOUS"
            if getattr(self, "_xstat_captured", False):
                when = "this call OR of a replay of a graph that captured evaluations of this engine since the last check; every such"
            raise RuntimeError(f"a pair hand-off inside a 256-channel transformer launch timed out (a partner workgroup was not "
                               f"scheduled within 0.3 s): the results of {when} call are invalid.  The pair-split launches need "
                               "their workgroups resident at the same time (compute units taken by another stream or process?); "
                               "set model.kernel_choice = 'wide' or MDT_TF256_PAIR=0 for forms without in-launch hand-offs")

    def handoff_status(self) -> int:
        """Diagnostic word of the pair hand-offs (synchronises): 0 = fine; bit 0 = some poll ran into its time-out, i.e. the
        results of that launch are garbage (a partner workgroup never arrived).  0 when the program has no pair-split op."""
        if getattr(self, "xflags", None) is None:
            return 0
        return int(self.xflags[0].item())

    # ------------------------------------------------------------------ per-call preparation
    def prepare_times(self, c_noise: torch.Tensor) -> None:
        """Time mapping + all FiLM (scale, shift) rows for every U-Net call of a sampling run at once
        (rows are identical across the batch: sigma is a scalar broadcast by to_batch, diffusion.py:91-102)."""
        n = c_noise.numel()
        if self.c.rows:
            raise RuntimeError("this engine holds the per-row programs (one time value per sample): use prepare_time_rows / eval_rows")
        if n > self.c.max_time_rows:
            raise ValueError(f"{n} U-Net evaluations per call (timesteps = {n // 2 + 1}) exceed the time table of "
                             f"{self.c.max_time_rows} rows this engine was compiled with (at most "
                             f"{self.c.max_time_rows // 2 + 1} timesteps); compile_unet(max_time_rows=...) sets it")
        off = self.c.shr["c_noise"]
        self.shr[off: off + n].copy_(c_noise.to(device=self.device, dtype=torch.float32), non_blocking=True)
        self.programs["time"].run(self._bind(), max(self.B, 1), n)
        self._time_rows = n

    def select_time(self, row: int) -> None:
        """Make row `row` of the precomputed FiLM table current for the next eval()."""
        assert 0 <= row < self._time_rows
        c = self.c
        src = c.shr["ss_all"] + row * c.ss_total
        dst = c.shr["ss_cur"]
        # one small launch of the library (a torch copy_ of the same bytes showed up as ~3 runtime copy kernels of ~4 us per evaluation
        # in the kernel trace, between the evaluation graphs; measured gain ~0.2 ms per 64-step call)
        base = self.shr.data_ptr()
        rt.check(rt.load_library().mdt_copy_f32(base + 4 * dst, base + 4 * src, c.ss_total, rt.current_stream()))

    def prepare_time_rows(self, c_noise_rows: torch.Tensor) -> None:
        """Per-row form: time mapping + all FiLM (scale, shift) rows for ONE evaluation with one c_noise value per sample of the
        reserved batch (KDiffusion_mod.forward / denoise_fn(sigmas=(B,)), diffusion.py:798-844).  The table has B rows in
        batch-scaled memory, so B is not limited by max_time_rows."""
        if not self.c.rows:
            raise RuntimeError("this engine holds the shared-row programs: compile_unet(rows=True) builds the per-row form")
        if c_noise_rows.numel() != self.B:
            raise ValueError(f"{c_noise_rows.numel()} time values for a reserved batch of {self.B}: the per-row form takes one per sample")
        off = self.c.act_named["c_noise"] * self.B
        self.act[off: off + self.B].copy_(c_noise_rows.to(device=self.device, dtype=torch.float32).flatten(), non_blocking=True)
        self.programs["time_rows"].run(self._bind(), self.B, self.B)

    def prepare_context(self, embedding: torch.Tensor) -> None:
        """Hoisted cross-attention K/V of every layer for this batch's conditioning embedding."""
        B = embedding.shape[0]
        self.reserve(B)
        emb = embedding.to(device=self.device, dtype=torch.float32).contiguous()
        assert emb.shape[1] == self.c.cond_len and emb.shape[2] == self.c.cfg.ctx_features, emb.shape
        self.programs["ctx"].run(self._bind(ctx=emb), B)

    def prepare_fixed(self) -> None:
        if not self._fixed_ready:
            self.programs["ctx_fixed"].run(self._bind(), max(self.B, 1))
            self._fixed_ready = True

    # ------------------------------------------------------------------ evaluation
    @property
    def has_dual(self) -> bool:
        """Both guidance passes as one evaluation of a doubled batch (program "eval_dual", see compiler.py)."""
        return "eval_dual" in self.programs

    def eval(self, fixed: bool = False, dual: bool = False) -> torch.Tensor:
        """One U-Net evaluation of self.xin for the whole batch -> self.pred (or self.pred_fixed).  dual: the batch is
        [conditional samples | the same samples again]; the second half attends to the fixed embedding."""
        name = "eval_dual" if dual else ("eval_fixed" if fixed else "eval")
        out = self.pred_fixed if fixed else self.pred
        if fixed or dual:
            self.prepare_fixed()
        if dual and (self.B % 2 or (self.B // 2) % self.c.dual_multiple):
            raise ValueError(f"the dual guidance batch needs 2 x (a multiple of {self.c.dual_multiple}) samples: a cross-attention "
                             "workgroup must not straddle the conditional and the unconditional half")
        return self._run_eval(name, out)

    def eval_rows(self, fixed: bool = False) -> torch.Tensor:
        """Per-row form: one U-Net evaluation of self.xin with the FiLM rows of prepare_time_rows -> self.pred (or
        self.pred_fixed, against the fixed embedding).  Same HIP-graph policy and hand-off handling as eval()."""
        if fixed:
            self.prepare_fixed()
        return self._run_eval("eval_rows_fixed" if fixed else "eval_rows", self.pred_fixed if fixed else self.pred)

    def _run_eval(self, name: str, out: torch.Tensor) -> torch.Tensor:
        if not self.use_graph:
            self.programs[name].run(self._bind(xin=self.xin, out=out), self.B)
            return out
        g = self._graphs.get(name)
        if g is None:
            # warm-up launch outside capture, then capture the ~350 launches of one evaluation
            self.programs[name].run(self._bind(xin=self.xin, out=out), self.B)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            # thread_local: only this thread's launches are captured; other threads (e.g. the RCCL watchdog of a
            # multi-GPU run) may keep issuing runtime calls without invalidating the capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.programs[name].run(self._bind(xin=self.xin, out=out), self.B)
            self._graphs[name] = g
        g.replay()
        return out
