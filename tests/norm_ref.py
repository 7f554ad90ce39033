"""Inputs and fp64 references for the LayerNorm / GroupNorm sections of csrc/ in the default (bf16x3) and exact (f32) modes, on
rows that leave mean 0.3 / std 1.5 (CPU, no GPU): what tests/test_gpu_norm_range.py compares the kernels with and
tests/test_norm_ref_host.py checks on the host.  DESIGN.md section 4.4.

Every case is ONE closed form `form(nm)` over a `Norm` -- the object that says how a statistic and an apply are evaluated -- and is
evaluated on exactly the operand bits the kernel reads:
  R    fp64, textbook: (x - mean) / sqrt(var_biased + eps) * gamma + beta, then FiLM, SiLU, the consuming product, residual;
  I    fp32 with torch on the CPU, the KERNEL'S OWN formula: two-pass variance; x * sc + (b - sc * mean) with sc = rstd * gamma
       where the site folds (FORMS below, read off the sources), (x - mean) * rstd * gamma + beta where it subtracts first;
  R16  R with both operands of every product rounded to hi + lo (softmax_ref.r16).
e_ref = max|I - R|, e16 = max|R16 - R|; the budget, the floor and the cap are softmax_ref's, unchanged."""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

import op_cases as oc
import softmax_ref as sr
from moleculediffusiontransformer_amd import runtime as rt
from softmax_ref import FLOOR, Refs, budget, cap_holds, check, ident, r16, ratio, rnd, ulp32      # noqa: F401  (the criterion, reused)

F64, F32 = torch.float64, torch.float32
FAMILIES = ["unit", "offset", "tiny", "huge", "mixed"]
EPS_MODEL = (1e-5, 1e-6)                  # the two values the model uses: ResNet GroupNorms and LayerNorms | Transformer1d.to_in
FAULTS = ["onepass", "eps_swap", "std_eps", "pooled", "clamped"]

# Which apply each site's source uses.  fold: x * sc + (b - sc * mean), sc = rstd * gamma; sub: (x - mean) * rstd [* gamma + beta]
# (a LayerNorm / to_in GroupNorm without affine has its gain and bias folded into the consuming weights by the compiler).
FORMS = {
    "k_gn_stats": "statistics only (two-pass)",                        # k_norm.hip:35-50
    "k_gemm LN": "sub", "k_gemm GN": "fold",                           # k_gemm.hip:189, :196-197
    "k_gemm_bf16x3 LN": "sub", "k_gemm_bf16x3 GN": "fold",             # k_gemm_bf16x3.hip:192, :205
    "k_gemm_as LN": "sub", "k_gemm_as GN": "fold",                     # k_gemm_as.hip:125-128, :141
    "k_gn_act": "fold",                                                # k_norm.hip:154-155
    "k_proj LN": "sub",                                                # k_proj.hip:184, :190
    "k_rconv GN": "fold",                                              # k_rconv.hip:386-387
    "k_resblock GN": "sub",                                            # k_resblock.hip:255, :334 (FiLM folded into gain / bias)
    "k_tblock_lw LN": "sub", "k_tblock32 LN": "sub",                   # k_tblock_lw.hip:236, k_tblock32.hip:300, :392
    "k_tf128 LN": "sub", "k_tf128 to_in GN": "sub", "k_tf128 ResNet GN": "fold",      # k_tf128.hip:452, :702, :528
    "k_tf256 LN": "sub", "k_tf256 to_in GN": "sub",                    # k_tf256.hip:798, :949 ff.
    "k_res256 GN": "fold",                                             # k_res256.hip:530
}


def f32(v):
    """The fp32 value a kernel receives for a Python float (eps, a skip scale)."""
    return float(torch.tensor(v, dtype=F32))


def other(eps):
    return EPS_MODEL[1] if eps == EPS_MODEL[0] else EPS_MODEL[0]


def silu(x):
    return x / (1.0 + torch.exp(-x))


class Norm:
    """How one evaluation of a closed form computes: dtype, operand rounding of the products, the apply (fold where the site
    folds, or never), the eps values by name, and at most one planted fault."""

    def __init__(self, eps, dt=F64, rr=ident, fold=False, fault=None, pad_rows=0):
        self.eps, self.dt, self.rr, self.fold, self.fault, self.pad_rows = dict(eps), dt, rr, fold, fault, pad_rows

    def t(self, x):
        return x.to(self.dt)

    def e(self, name):
        v = self.eps[name]
        return f32(other(v) if self.fault == "eps_swap" else v)

    # ---- statistics of units: xu [..., U, n], one (mean, rstd) per unit ----
    def stats(self, xu, eps):
        if self.fault == "pooled":                    # unit u shares its statistics with its neighbour u ^ 1
            U = xu.shape[-2]
            partner = (torch.arange(U) ^ 1).clamp(max=U - 1)
            xu = torch.cat([xu, xu[..., partner, :]], -1)
        mean = xu.mean(-1, keepdim=True)
        if self.fault == "onepass":
            var = ((xu * xu).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
        else:
            var = ((xu - mean) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / (var.sqrt() + eps) if self.fault == "std_eps" else 1.0 / torch.sqrt(var + eps)
        return mean, rstd

    def ln(self, x, g, b, name="eps"):
        """LayerNorm over the last dimension, subtract-first; g / b None: no affine."""
        x = self.t(x)
        mean, rstd = self.stats(x.reshape(-1, x.shape[-1]), self.e(name))
        y = (x - mean.view(*x.shape[:-1], 1)) * rstd.view(*x.shape[:-1], 1)
        return y if g is None else y * self.t(g) + self.t(b)

    def gn_stats(self, x, G, name="eps"):
        """x [B, T, C] -> mean, rstd [B, G] over each (sample, group)'s T * C / G values."""
        x = self.t(x)
        B, T, C = x.shape
        gs = C // G

        def units(t):                                  # [b, rows, C] -> [b, G, rows * gs]
            return t.view(t.shape[0], t.shape[1], G, gs).permute(0, 2, 1, 3).reshape(t.shape[0], G, -1)
        xu = units(x)
        mean, rstd = self.stats(xu.view(1, B, -1) if G == 1 else xu, self.e(name))       # (G = 1: the neighbour is a sample)
        mean, rstd = mean.view(B, G).clone(), rstd.view(B, G).clone()
        if self.fault == "clamped" and self.pad_rows:   # the last sample's statistics over the duplicates of its last row too
            last = torch.cat([x[-1:], x[-1:, -1:].expand(1, self.pad_rows, C)], 1)
            m, r = self.stats(units(last), self.e(name))
            mean[-1], rstd[-1] = m.view(G), r.view(G)
        return mean, rstd

    def gn(self, x, G, g, b, name="eps", fold=True):
        """GroupNorm of x [B, T, C] (channels last).  fold: the site applies x * sc + (b - sc * mean)."""
        x = self.t(x)
        B, T, C = x.shape
        mean, rstd = self.gn_stats(x, G, name)
        mean = mean.repeat_interleave(C // G, 1).view(B, 1, C)
        rstd = rstd.repeat_interleave(C // G, 1).view(B, 1, C)
        if g is None:
            return (x - mean) * rstd
        if fold and self.fold:
            sc = rstd * self.t(g)
            return x * sc + (self.t(b) - sc * mean)
        return (x - mean) * rstd * self.t(g) + self.t(b)

    def mm(self, a, w):
        """a [.., K] times w [N, K]^T."""
        return self.rr(a) @ self.rr(self.t(w)).transpose(-1, -2)

    def conv(self, h, w, init=None):
        """Conv1d(k = 1 | 3, zero padding) of h [B, T, Cin] (channels last) with w [Cout, Cin, k].  init: what the kernel's
        accumulators START from (the bias, the residual stream): k_tf128 RES, k_res256 and k_resblock set the accumulators to it
        and add the products MFMA by MFMA, so every partial sum is rounded at the magnitude of init.  The fp32 form does the same in
        steps of 4 products, the K of one exact-mode MFMA; in fp64 the order does not matter."""
        w = self.t(w)
        k = w.shape[2]
        if init is None or self.dt is F64:
            y = F.conv1d(self.rr(h).transpose(1, 2), self.rr(w), None, padding=k // 2).transpose(1, 2)
            return y if init is None else y + self.t(init)
        T = h.shape[1]
        hp = F.pad(h, (0, 0, k // 2, k // 2))
        acc = self.t(init).expand(h.shape[0], T, w.shape[0]).clone()
        for tap in range(k):
            for c0 in range(0, w.shape[1], 4):
                acc = acc + hp[:, tap: tap + T, c0: c0 + 4] @ w[:, c0: c0 + 4, tap].T
        return acc

    def film(self, y, ss, C, ld=None):
        ss = self.t(ss)
        return y * (ss[:C] + 1.0) + ss[(ld or C): (ld or C) + C]


# ---- input families ---------------------------------------------------------------------------------------------------------------
# A unit is what one (mean, rstd) pair covers.  `mag` scales a family's departure from `unit` (1 = as DESIGN.md 4.4 states it;
# MAGNITUDE below halves it for a site whose references alone would break the cap).

def _unit(n_units, n, seed):
    return rnd(n_units, n, seed=seed) * 1.5 + 0.3


def family_units(family, cls, n, seed, mag=1.0):
    """[U, n] fp32 values, one row per unit.  cls [U]: the unit's scale class, used by `mixed` alone (0: unit * 2^12, 1: unit *
    2^-12, 2: all zeros, 3: offset)."""
    U = cls.numel()
    u = _unit(U, n, seed)
    off = rnd(U, n, seed=seed + 1000) + 64.0 * mag
    if family == "unit":
        return u
    if family == "offset":
        return off
    if family == "tiny":
        return rnd(U, n, seed=seed) * (2.0 ** -10 * mag)
    if family == "huge":
        return u * (4096.0 * mag)
    assert family == "mixed", family
    out = torch.zeros(U, n)
    out[cls == 0] = u[cls == 0] * (4096.0 * mag)
    out[cls == 1] = u[cls == 1] * (2.0 ** -12 / mag)
    out[cls == 3] = off[cls == 3]
    return out


def ln_classes(M):
    """Scale class of each of M rows: the cycle runs over the rows and ends on an all-zero row, so that the last valid row of a
    partial tile is one."""
    return (torch.arange(M) + 2 - (M - 1)) % 4


def gn_classes(B, G):
    """Scale class of each (sample, group): the cycle runs over the groups with another phase in every sample."""
    return (torch.arange(G).view(1, G) + torch.arange(B).view(B, 1)) % 4


PRESENT = "present"        # not a family: the inputs the builders of tests/op_cases.py have always had (the host test's "old" column)


def ln_input(family, M, C, seed=4, mag=1.0):
    return None if family == PRESENT else family_units(family, ln_classes(M), C, seed, mag)


def gn_input(family, B, T, C, G, seed=4, mag=1.0):
    """[B, T, C]: every (sample, group) is one unit of T * C / G values."""
    if family == PRESENT:
        return None
    gs = C // G
    u = family_units(family, gn_classes(B, G).reshape(-1), T * gs, seed, mag)
    return u.view(B, G, T, gs).permute(0, 2, 1, 3).reshape(B, T, C).contiguous()


# (site, family) -> magnitude: a family is halved for a site until the cap holds for all its cases (test_norm_ref_host checks the
# cap; DESIGN.md 4.4 records the values).  Nothing needed halving.
MAGNITUDE = {}


def mag_of(site, family):
    return MAGNITUDE.get((site, family), 1.0)


# ---- a case -----------------------------------------------------------------------------------------------------------------------

class Case:
    """site / shape / family / eps (name -> value used), form(nm) -> the output in the shape of R, lower(prod) -> (ops, weights, act,
    shr, ext, B, out, untouched, regions): out(act') = the result in the shape of R, untouched = [lo, hi) ranges of act that hold
    inputs, regions = per-sample float counts of the arena's tensors in order (act = cat of B * n_k floats).  ring: a ring kernel
    (both product modes); split: None = follows prod, else fixed.  gn: a GroupNorm site (the fold has a price); pad_rows: duplicate
    rows of a partial 16-row tile."""

    def __init__(self, site, shape, family, eps, form, lower, ring=False, split=False, gn=False, pad_rows=0, kernel=None, rows=0):
        self.site, self.shape, self.family, self.eps, self.form, self.lower = site, shape, family, eps, form, lower
        self.ring, self.split, self.gn, self.pad_rows, self.kernel = ring, split, gn, pad_rows, kernel or site
        self.rows = rows                   # token rows of a sample where a GroupNorm unit spans the rows of a 16-row tile

    @property
    def key(self):
        e = ",".join(f"{k}={v:g}" for k, v in self.eps.items())
        return f"{self.site} {self.shape} {self.family} {e}"

    def prods(self):
        return ["bf16x3", "f32"] if self.ring else [None]

    def is_split(self, prod):
        return prod == "bf16x3" if self.ring else self.split

    def eval(self, dt=F64, rr=ident, fold=True, fault=None, eps=None):
        return self.form(Norm(eps or self.eps, dt, rr, fold, fault, self.pad_rows))

    @functools.cached_property
    def refs(self):
        R, I, R16 = self.eval(), self.eval(F32), self.eval(rr=r16)
        return Refs(R, I, R16, (I.double() - R).abs().max().item(), (R16 - R).abs().max().item(), 0.0)

    @functools.cached_property
    def e_ref_subtract_first(self):
        """e_ref with I in the subtract-first form: what the references would disagree by if the site did not fold."""
        return (self.eval(F32, fold=False).double() - self.refs.R).abs().max().item()

    def eps_shift(self, name):
        """max|R' - R| in fp64 when eps `name` alone takes the other model value."""
        return (self.eval(eps={**self.eps, name: other(self.eps[name])}) - self.refs.R).abs().max().item()


def eps_variants(prod_eps):
    """The site's production values, and every one of them replaced by the other model value."""
    return [dict(prod_eps), {k: other(v) for k, v in prod_eps.items()}]


def _set_eps(op, eps, slots):
    for name, slot in slots.items():
        op.f[slot] = eps[name]


# ---- MDT_OP_GN_STATS and the GEMM prologues ---------------------------------------------------------------------------------------

GN_SHAPES = [(5, 4, 512, 8), (3, 64, 64, 1), (2, 32, 32, 32)]                    # (B, R, C, G)
GN_GEMM = {(5, 4, 512, 8): (256, True, True), (3, 64, 64, 1): (64, False, True), (2, 32, 32, 32): (32, False, False)}   # N, FiLM, SiLU
GN_PROD_EPS = {(5, 4, 512, 8): 1e-5, (3, 64, 64, 1): 1e-5, (2, 32, 32, 32): 1e-6}


def gn_stats_case(shape, family, eps, what):
    """k_gn_stats<64 | 256> read back from the arena; what = 'mean' | 'rstd' (each held to its own scale)."""
    B, R, C, G = shape
    N, film, do_silu = GN_GEMM[shape]
    x = gn_input(family, B, R, C, G, mag=mag_of("k_gn_stats", family))
    c = oc.groupnorm_gemm(B, R, C, G, N, film, do_silu, eps["eps"], x=x)
    col = 0 if what == "mean" else 1

    def form(nm):
        return nm.gn_stats(x, G)[col]

    def lower(prod):
        def out(a):
            return a[B * c.stoff: B * c.stoff + B * 2 * G].view(B, G, 2)[:, :, col]
        return [c.ops[0]], c.weights, c.act, c.shr, {}, B, out, [(0, B * R * C)], [R * C, 64, R * N]
    k = "k_gn_stats<64>" if R * (C // G) <= 256 else "k_gn_stats<256>"
    return Case(f"k_gn_stats {what}", shape, family, eps, form, lower, kernel=k)


def gemm_gn_case(shape, family, eps):
    B, R, C, G = shape
    N, film, do_silu = GN_GEMM[shape]
    x = gn_input(family, B, R, C, G, mag=mag_of("k_gemm GN", family))
    c = oc.groupnorm_gemm(B, R, C, G, N, film, do_silu, eps["eps"], x=x)
    x = c.act[: B * R * C].view(B, R, C)
    w3 = c.w.view(N, c.taps, C).permute(0, 2, 1)

    def form(nm):
        h = nm.gn(x, G, c.g, c.b)
        if film:
            h = nm.film(h, c.shr, C)
        return nm.conv(silu(h) if do_silu else h, w3)

    def lower(prod):
        return c.ops, c.weights, c.act, c.shr, {}, B, (lambda a: a[B * c.ooff:].view(B, R, N)), [(0, B * R * C)], [R * C, 64, R * N]
    return Case("k_gemm GN", shape, family, eps, form, lower, gn=True)


LN_GEMM_SHAPES = [(3, 12, 128, 1024), (130, 1, 64, 64)]                          # (B, R, C, N)


def gemm_ln_case(shape, family, eps):
    B, R, C, N = shape
    x = ln_input(family, B * R, C, mag=mag_of("k_gemm LN", family))
    c = oc.layernorm_gemm(B, R, C, N, x=x, eps=eps["eps"])
    x = c.act[: B * R * C].view(B * R, C)

    def form(nm):
        return nm.mm(nm.ln(x, c.g, c.b), c.w)

    def lower(prod):
        return c.ops, c.weights, c.act, c.shr, {}, B, (lambda a: a[B * R * C:].view(B * R, N)), [(0, B * R * C)], [R * C, R * N]
    return Case("k_gemm LN", shape, family, eps, form, lower)


# (B, R, cin, N, taps): k_gemm3 with 64x64 tiles and conv taps, the A-stationary kernel, one row per sample with a ragged N.  A
# LayerNorm prologue takes its row statistics at one tap (k_gemm_bf16x3.hip ln_prepass), so the LayerNorm cases run k = 1.
SPLIT_SHAPES = [(3, 16, 128, 96, 3), (40, 4, 256, 256, 1), (33, 1, 256, 160, 1)]


def split_gemm_case(shape, family, eps, pro):
    B, R, cin, N, taps = shape
    gnorm = pro == rt.PRO_GROUPNORM
    if not gnorm:
        taps = 1
    kernel = "k_gemm_as" if shape[:2] == (40, 4) else "k_gemm_bf16x3"
    site = f"{kernel} {'GN' if gnorm else 'LN'}"
    if gnorm:
        x = gn_input(family, B, R, cin, 8, seed=5, mag=mag_of(site, family))
    else:
        x = ln_input(family, B * R, cin, seed=5, mag=mag_of(site, family))
    c = oc.split_gemm(B, R, cin, N, taps, pro, x=x, eps=eps["eps"])
    x = c.act[: B * R * cin].view(B, R, cin)
    w16 = r16(c.w)                                       # the planes hold hi and lo: the kernel reads exactly hi + lo
    w3 = w16.view(N, taps, cin).permute(0, 2, 1)
    res = c.res.view(B, R, N)

    def form(nm):
        if gnorm:
            h = silu(nm.film(nm.gn(x, c.G, c.g, c.b), c.shr, cin))
        else:
            h = nm.ln(x, c.g, c.b)
        return nm.conv(h, w3) + nm.t(c.bias) + nm.t(res)

    def lower(prod):
        return (c.ops, c.weights, c.act, c.shr, {}, B, (lambda a: a[B * c.ooff: B * c.roff].view(B, R, N)),
                [(0, B * R * cin), (B * c.roff, c.act.numel())], [R * cin, 64, R * N, R * N])
    return Case(site, shape[:4] + (taps,), family, eps, form, lower, split=True, gn=gnorm, kernel=kernel)


# ---- k_gn_act ----------------------------------------------------------------------------------------------------------------------

# (B, R, C, G, FiLM, SiLU, production eps): one shape per reachable dispatch branch of launch_gn_act (tests/test_gpu_poison.py)
GN_ACT_SHAPES = [(2, 4, 256, 32, False, False, 1e-6), (3, 16, 128, 8, True, True, 1e-5), (5, 64, 64, 1, False, True, 1e-5),
                 (2, 64, 128, 1, False, True, 1e-5), (2, 16, 512, 8, True, True, 1e-5), (3, 32, 512, 8, True, True, 1e-5),
                 (2, 32, 1024, 8, False, True, 1e-5), (2, 128, 256, 4, False, True, 1e-5), (3, 32, 512, 32, False, False, 1e-6),
                 (2, 48, 512, 32, False, False, 1e-6)]
GN_ACT2_SHAPES = [(3, 4, 64, 4, 0.7071), (37, 8, 1024, 8, 0.5)]                  # (B, R, C, G, SCALE2): two sources, fp32 output


def gn_act_case(shape, family, eps):
    B, R, C, G, film, do_silu, _ = shape
    x = gn_input(family, B, R, C, G, mag=mag_of("k_gn_act", family))
    c = oc.gn_act(B, R, C, G, film, do_silu, eps["eps"], x=x)
    x = c.act[: B * R * C].view(B, R, C)

    def form(nm):
        h = nm.gn(x, G, c.g, c.b)
        if film:
            h = nm.film(h, c.shr, C)
        return silu(h) if do_silu else h

    def lower(prod):
        return c.ops, c.weights, c.act, c.shr, {}, B, (lambda a: a[B * R * C:].view(B, R, C)), [(0, B * R * C)], [R * C, R * C]
    case = Case("k_gn_act", shape[:6], family, eps, form, lower, gn=True)
    case.x, case.beta, case.G = x, c.b, G
    return case


def gn_act2_case(shape, family, eps):
    B, R, C, G, scale2 = shape
    ld = 2 * C
    xcat = gn_input(family, B, R, ld, G, mag=mag_of("k_gn_act two sources", family))
    xa, xb = xcat[:, :, :C].contiguous(), xcat[:, :, C:].contiguous()
    c = oc.gn_act_two_sources(B, R, C, G, scale2=scale2, out16=False, xa=xa, xb=xb, eps=eps["eps"])

    def form(nm):
        return silu(nm.gn(torch.cat([nm.t(xa), nm.t(xb) * f32(scale2)], 2), G, c.g, c.b))

    def lower(prod):
        return (c.ops, c.weights, c.act, c.shr, {}, B, (lambda a: a[B * c.yoff:].view(B, R, ld)), [(0, B * c.yoff)],
                [R * C, R * C, R * ld])
    return Case("k_gn_act two sources", shape, family, eps, form, lower, gn=True, kernel="k_gn_act")


# ---- the ring kernels: k_proj, k_rconv, k_resblock ----------------------------------------------------------------------------------

PROJ_SHAPES = [(37, 1, 256, 1024, "plain", True), (37, 1, 256, 1024, "affine", False),
               (5, 4, 128, 64, "plain", True), (5, 4, 128, 64, "affine", False)]     # (B, R, cin, N, LayerNorm, residual)


def proj_case(shape, family, eps, B_rows=None):
    B, R, cin, N, ln, res = shape
    x = ln_input(family, B * R, cin, seed=3, mag=mag_of("k_proj LN", family))
    if x is None:
        x = oc.ring_projection(B, R, cin, N, ln, res, "f32").x.view(B * R, cin)
    if B_rows is not None:                               # a sub-batch: these samples alone
        x = x.view(B, R * cin)[B_rows].reshape(-1, cin)
        B = len(B_rows)
    built = {}

    def c(prod):
        if prod not in built:
            built[prod] = oc.ring_projection(B, R, cin, N, ln, res, prod or "f32", x=x, eps=eps["eps"])
        return built[prod]

    def form(nm):
        p = c(None)
        y = nm.mm(nm.ln(x, p.g, p.b) if ln == "affine" else nm.ln(x, None, None), p.w) + nm.t(p.bias)
        return y + nm.t(p.out0.view(B * R, N)) if res else y

    def lower(prod):
        p = c(prod)
        return [p.ops[0]], p.weights, p.act, p.shr, {}, B, (lambda a: a[B * R * cin:].view(B * R, N)), [(0, B * R * cin)], [R * cin, R * N]
    return Case("k_proj LN", shape, family, eps, form, lower, ring=True, kernel="k_proj")


# (C, T, B, taps, gsize, FiLM, SiLU, residual, in_scale)
RCONV_SHAPES = [(128, 16, 5, 3, 16, True, True, "other", 1.0), (256, 4, 9, 3, 64, False, True, "accumulate", 0.7071),
                (256, 1, 33, 3, 32, False, True, None, 1.0)]
RCONV2_SHAPES = [(256, 4, 37, 3, 64, True, 0.7071)]                              # (C, T, B, taps, gsize, SiLU, in_scale2)


def _pad16(rows):
    return (-rows) % 16


def rconv_case(shape, family, eps, B_rows=None):
    C, T, B, taps, gsize, film, do_silu, res, in_scale = shape
    G = C // gsize
    x = gn_input(family, B, T, C, G, mag=mag_of("k_rconv GN", family))
    if x is None:
        x = oc.ring_conv(C, T, B, taps, gsize, film, do_silu, res, in_scale, "f32").act[: B * T * C].view(B, T, C)
    if B_rows is not None:
        x, B = x[B_rows].contiguous(), len(B_rows)
    built = {}

    def c(prod):
        if prod not in built:
            built[prod] = oc.ring_conv(C, T, B, taps, gsize, film, do_silu, res, in_scale, prod or "f32", x=x, eps=eps["eps"])
        return built[prod]
    n = B * T * C

    def form(nm):
        p = c(None)
        h = nm.gn(nm.t(x) * f32(in_scale), G, p.gb[:C], p.gb[C: 2 * C])
        if film:
            h = nm.film(h, p.shr, C)
        y = nm.conv(silu(h) if do_silu else h, p.w)
        if res != "accumulate":
            y = y + nm.t(p.gb[2 * C:])
        if res:
            y = y + nm.t((p.act[2 * n:] if res == "other" else p.act[n: 2 * n]).view(B, T, C))
        return y

    def lower(prod):
        p = c(prod)
        return [p.ops[0]], p.weights, p.act, p.shr, {}, B, (lambda a: a[n: 2 * n].view(B, T, C)), [(0, n), (2 * n, 3 * n)], [T * C] * 3
    return Case("k_rconv GN", shape, family, eps, form, lower, ring=True, gn=True, pad_rows=_pad16(B * T), kernel="k_rconv", rows=T)


def rconv2_case(shape, family, eps):
    C, T, B, taps, gsize, do_silu, in_scale2 = shape
    G = 2 * C // gsize
    xcat = gn_input(family, B, T, 2 * C, G, mag=mag_of("k_rconv GN, two sources", family))
    xa, xb = xcat[:, :, :C].contiguous(), xcat[:, :, C:].contiguous()
    built = {}

    def c(prod):
        if prod not in built:
            built[prod] = oc.ring_conv_two_sources(C, T, B, taps, gsize, do_silu, in_scale2, prod or "f32", xa=xa, xb=xb, eps=eps["eps"])
        return built[prod]
    n = B * T * C

    def form(nm):
        p = c(None)
        h = nm.gn(torch.cat([nm.t(xa), nm.t(xb) * f32(in_scale2)], 2), G, p.gb[: 2 * C], p.gb[2 * C: 4 * C])
        return nm.conv(silu(h) if do_silu else h, p.w) + nm.t(p.gb[4 * C:])

    def lower(prod):
        p = c(prod)
        return [p.ops[0]], p.weights, p.act, p.shr, {}, B, (lambda a: a[n: 2 * n].view(B, T, C)), [(0, n), (2 * n, 3 * n)], [T * C] * 3
    return Case("k_rconv GN, two sources", shape, family, eps, form, lower, ring=True, gn=True, pad_rows=_pad16(B * T), kernel="k_rconv", rows=T)


RESBLOCK_SHAPES = [(5, 50, 7, True), (2, 16, 7, True), (16, 1, 1, True)]         # (cin, cout, B, FiLM); 64 tokens, one group
# tiny_mid: the first convolution times 2^-10 -- the SECOND GroupNorm meets tiny; offset_mid: 64 added to its bias -- the second
# GroupNorm meets offset, while the block's own 1x1 convolution of the raw input (which at `offset` sets the scale of the output,
# |R|max 120 - 180, and of e16) sees unit rows
RESBLOCK_FAMILIES = FAMILIES + ["tiny_mid", "offset_mid"]
MID_FAMILIES = {"tiny_mid": (2.0 ** -10, 0.0), "offset_mid": (1.0, 64.0)}


def resblock_case(shape, family, eps, B_rows=None):
    cin, cout, B, film = shape
    T = 64
    scale1, shift1 = MID_FAMILIES.get(family, (1.0, 0.0))
    fam = "unit" if family in MID_FAMILIES else family
    x = gn_input(fam, B, T, cin, 1, seed=12, mag=mag_of("k_resblock GN", fam))
    if B_rows is not None:
        x, B = x[B_rows].contiguous(), len(B_rows)
    cin_p, cout_p = (cin + 15) // 16 * 16, (cout + 15) // 16 * 16
    built = {}

    def c(prod):
        if prod not in built:
            comp, op, shr, _, sd = oc.resblock_case(cin, cout, film, prod or "f32", scale1, shift1)
            op.f[0] = eps["eps"]
            built[prod] = NS(op=op, weights=comp.W.pack(), shr=shr, sd=sd)
        return built[prod]
    xin = torch.zeros(B, T, cin_p)
    xin[:, :, :cin] = x
    n_in, n_out = B * T * cin_p, B * T * cout_p
    act = torch.cat([xin.view(-1), torch.full((n_out,), 7.0)])

    def form(nm):
        p = c(None)
        sd, q = p.sd, "blk."
        h = nm.conv(silu(nm.gn(x, 1, sd[q + "block1.groupnorm.weight"], sd[q + "block1.groupnorm.bias"], fold=False)),
                    sd[q + "block1.project.weight"], init=sd[q + "block1.project.bias"])
        h = nm.gn(h, 1, sd[q + "block2.groupnorm.weight"], sd[q + "block2.groupnorm.bias"], fold=False)
        if film:
            h = nm.film(h, p.shr, cout, cout_p)
        y = nm.conv(silu(h), sd[q + "block2.project.weight"]) + nm.t(sd[q + "block2.project.bias"])
        return y + nm.conv(nm.t(x), sd[q + "to_out.weight"]) + nm.t(sd[q + "to_out.bias"])

    def lower(prod):
        p = c(prod)

        def out(a):
            o = a[n_in:].view(B, T, cout_p)
            assert (o[:, :, cout:] == 0).all(), "the padded output channels hold exact zeros"
            return o[:, :, :cout]
        return [p.op], p.weights, act, p.shr, {}, B, out, [(0, n_in)], [T * cin_p, T * cout_p]
    return Case("k_resblock GN", shape, family, eps, form, lower, ring=True, gn=True, kernel="k_resblock")


# ---- the attention sub-blocks and the whole-level kernels -------------------------------------------------------------------------

H, D, MID, N_CTX = sr.H, sr.D, sr.MID, sr.N_CTX


def _attention(nm, h, sd, p, kv):
    """h + Attention(h) of the reference's module (modules.py:401-410, :350-364) over a Norm."""
    def g(n):
        return sd[p + n]
    B, T, C = h.shape
    xn = nm.ln(h, g("norm.weight"), g("norm.bias"), "eps_ln")
    q = nm.mm(xn, g("to_q.weight")).view(B, T, H, D).transpose(1, 2)
    if kv is None:
        kv = nm.mm(nm.ln(h, g("norm_context.weight"), g("norm_context.bias"), "eps_ln"), g("to_kv.weight"))
    k, v = nm.t(kv).chunk(2, dim=-1)
    k = k.reshape(B, -1, H, D).transpose(1, 2)
    v = v.reshape(B, -1, H, D).transpose(1, 2)
    s = nm.rr(q) @ nm.rr(k).transpose(-1, -2) * 0.125
    o = (nm.rr(s.softmax(-1)) @ nm.rr(v)).transpose(1, 2).reshape(B, T, MID)
    return h + nm.mm(o, g("attention.to_out.weight")) + nm.t(g("attention.to_out.bias"))


def _transformer(nm, x, sd, p, layers, cross, kv):
    """Transformer1d of the reference (modules.py:469-524): GroupNorm(32, eps_gn) + 1x1 to_in, the layers, the 1x1 to_out."""
    def g(n):
        return sd[p + n]
    h = nm.gn(x, 32, g("to_in.0.weight"), g("to_in.0.bias"), "eps_gn", fold=False)
    h = nm.mm(h, g("to_in.1.weight")[:, :, 0]) + nm.t(g("to_in.1.bias"))
    for li in range(layers):
        bp = p + f"blocks.{li}."
        h = _attention(nm, h, sd, bp + "attention.", None)
        if cross:
            h = _attention(nm, h, sd, bp + "cross_attention.", kv[li])
        f_ = f"blocks.{li}.feed_forward."
        h = h + nm.mm(F.gelu(nm.mm(h, g(f_ + "0.weight")) + nm.t(g(f_ + "0.bias"))), g(f_ + "2.weight")) + nm.t(g(f_ + "2.bias"))
    return nm.mm(h, g("to_out.1.weight")[:, :, 0]) + nm.t(g("to_out.1.bias"))


# (kernel, variant, C, T, B): MDT_OP_TBLOCK; each as a self- and as a cross-attention block where the variant serves cross blocks
# of 12 context rows at that T (variant 0: at most 16 keys per 16 rows).  The feed-forward block has no normalisation.
TBLOCK_SHAPES = [("k_tblock32", 2, 256, 4, 37), ("k_tblock_lw", 0, 128, 1, 70), ("k_tblock_lw", 0, 128, 16, 5)]


def tblock_modes(variant, T):
    keys = (16 // T) * N_CTX
    return [rt.TB_SELF] + ([rt.TB_CROSS] if keys <= (16 if variant == 0 else 48) else [])


def tblock_case(shape, mode, family, eps, B_rows=None):
    kernel, variant, C, T, B = shape
    base = sr.tblock_case(variant, mode, C, T, B)
    x = ln_input(family, B * T, C, seed=13, mag=mag_of(f"{kernel} LN", family)).view(B, T, C)
    kv = base["kv"].view(B, N_CTX, 2 * MID)
    if B_rows is not None:
        x, kv, B = x[B_rows].contiguous(), kv[B_rows].contiguous(), len(B_rows)
    c = dict(base, x=x.reshape(-1), kv=kv.reshape(-1), B=B)
    sd, p = base["sd"], base["p"]

    def form(nm):
        return _attention(nm, nm.t(x), sd, p, kv if mode == rt.TB_CROSS else None)

    def lower(prod):
        ops, weights, act, shr, ext, B_, out, untouched = sr.lower_tblock(c, 1, prod)
        ops[0].f[0] = eps["eps_ln"]
        return ops, weights, act, shr, ext, B_, out, untouched, [T * C, N_CTX * 2 * MID]
    name = "self" if mode == rt.TB_SELF else "cross"
    return Case(f"{kernel} LN", (variant, C, T, B, name), family, eps, form, lower, ring=True, kernel=kernel)


# (kernel, C, T, B, layers, cross, form)
TF_SHAPES = [("k_tf128", 128, 2, 33, 1, False, "whole"), ("k_tf256", 256, 4, 37, 2, True, "whole"),
             ("k_tf256", 256, 4, 37, 2, True, "pair8")]
# the families on the kernel's input reach its FIRST norm, to_in's GroupNorm; tiny_ln: to_in's convolution times 2^-10, so that the
# first LayerNorms (self-attention: norm and norm_context) meet rows of std 2^-10 around a mean of 2^-10 * bias
TF_FAMILIES = FAMILIES + ["tiny_ln"]
TF_EPS = {"eps_ln": 1e-5, "eps_gn": 1e-6}


def tf_case(shape, family, eps, B_rows=None):
    kernel, C, T, B, layers, cross, form_ = shape
    base = sr.tf_case(C, T, B, layers, cross)
    fam = "unit" if family == "tiny_ln" else family
    x = gn_input(fam, B, T, C, 32, seed=13, mag=mag_of(f"{kernel} to_in GN", fam))
    sd, p = dict(base["sd"]), base["p"]
    if family == "tiny_ln":
        sd[p + "to_in.1.weight"], sd[p + "to_in.1.bias"] = sd[p + "to_in.1.weight"] * 2.0 ** -10, sd[p + "to_in.1.bias"] * 2.0 ** -10
    kv = base["kv"].view(layers, B, N_CTX, 2 * MID) if cross else None
    if B_rows is not None:
        x, B = x[B_rows].contiguous(), len(B_rows)
        kv = kv[:, B_rows].contiguous() if cross else None
    c = dict(base, x=x.reshape(-1), sd=sd, B=B, kv=kv.reshape(-1) if cross else base["kv"])

    def form(nm):
        return _transformer(nm, nm.t(x), sd, p, layers, cross, kv)

    def lower(prod):
        ops, weights, act, shr, ext, B_, out, untouched = sr.lower_tf(c, 1, prod, form_)
        _set_eps(ops[0], eps, {"eps_ln": rt.FF_EPS_LN, "eps_gn": rt.FF_EPS_GN})
        return ops, weights, act, shr, ext, B_, out, untouched, [T * C, T * C] + [N_CTX * 2 * MID] * (layers if cross else 0)
    return Case(f"{kernel} LN, to_in GN", (C, T, B, layers, "cross" if cross else "self", form_), family, eps, form, lower,
                ring=True, pad_rows=_pad16(B * T), kernel=kernel, rows=T)


def _res_chain(nm, x, sk, sd, blocks, kind, G, film, C, name):
    """ResnetBlock1d blocks in a row (modules.py:145-205; :828-829: cat with the scaled skip), GroupNorms folded as the kernels do."""
    h, n_res = nm.t(x), len(blocks)
    for k, bp in enumerate(blocks):
        fl = nm.t(film[k * 2 * C: (k + 1) * 2 * C])
        xin = h
        if kind == 2:
            xin = torch.cat([h, nm.t(sk[n_res - 1 - k]) * f32(2 ** -0.5)], 2)
        t1 = nm.conv(silu(nm.gn(xin, G, sd[bp + "block1.groupnorm.weight"], sd[bp + "block1.groupnorm.bias"], name)),
                     sd[bp + "block1.project.weight"], init=sd[bp + "block1.project.bias"])
        t2 = nm.gn(t1, G, sd[bp + "block2.groupnorm.weight"], sd[bp + "block2.groupnorm.bias"], name)
        # the block's output accumulates on its residual: the stream, or to_out(cat) and its bias (k_res256.hip:743, :766-768)
        acc = nm.t(sd[bp + "block2.project.bias"]) + (xin if kind == 1 else nm.t(sd[bp + "to_out.bias"]))
        if kind == 2:
            acc = nm.conv(xin, sd[bp + "to_out.weight"], init=acc)
        h = nm.conv(silu(t2 * (fl[:C] + 1.0) + fl[C:]), sd[bp + "block2.project.weight"], init=acc)
    return h


def _mid(blocks, family):
    """tiny_mid: every block's first convolution times 2^-10 -- its second GroupNorm meets values of std ~2^-10; offset_mid: 64 added
    to its bias -- the second GroupNorm meets a mean of 64."""
    if family not in MID_FAMILIES:
        return None
    scale1, shift1 = MID_FAMILIES[family]

    def edit(sd):
        for bp in blocks:
            sd[bp + "block1.project.weight"] = sd[bp + "block1.project.weight"] * scale1
            sd[bp + "block1.project.bias"] = sd[bp + "block1.project.bias"] * scale1 + shift1
    return edit


RES_FAMILIES = FAMILIES + ["tiny_mid", "offset_mid"]
RES128_SHAPES = [(1, 4, 18, 2, 1), (2, 8, 9, 2, 1)]                              # (kind, T, B, n_res, layers): MDT_OP_TF128
RES128_EPS = {"eps_res": 1e-5, "eps_ln": 1e-5, "eps_gn": 1e-6}


def _res_inputs(site, family, kind, B, T, C, G, n_res):
    fam = "unit" if family in MID_FAMILIES else family
    if kind == 1:
        return gn_input(fam, B, T, C, G, seed=13, mag=mag_of(site, fam)), None
    xcat = gn_input(fam, B, T, 2 * C, G, seed=13, mag=mag_of(site, fam))          # the first block's cat([x, skip]): 2 C channels
    sk = torch.stack([gn_input(fam, B, T, 2 * C, G, seed=16 + 7 * k, mag=mag_of(site, fam))[:, :, C:] for k in range(n_res)])
    sk[n_res - 1] = xcat[:, :, C:]                                                # (skips are consumed from the last downwards)
    return xcat[:, :, :C].contiguous(), sk.contiguous()


def res128_case(shape, family, eps, B_rows=None):
    kind, T, B, n_res, layers = shape
    C, G = 128, 8
    site = "k_tf128 ResNet GN"
    x, sk = _res_inputs(site, family, kind, B, T, C, G, n_res)
    if B_rows is not None:
        x, sk, B = x[B_rows].contiguous(), (None if sk is None else sk[:, B_rows].contiguous()), len(B_rows)
    blocks = [f"res{k}." for k in range(n_res)]
    built = {}

    def c(prod):
        if prod not in built:
            built[prod] = oc.resnets_in_tf128(kind, T, B, n_res, layers, False, prod or "f32", x=x, sk=sk,
                                              sd_edit=_mid(blocks, family))
            _set_eps(built[prod].ops[0], eps, {"eps_ln": rt.FF_EPS_LN, "eps_gn": rt.FF_EPS_GN, "eps_res": rt.FF_EPS_RES})
        return built[prod]
    n = B * T * C

    def form(nm):
        p = c(None)
        h = _res_chain(nm, x, sk, p.sd, blocks, kind, G, p.shr[oc.FILM_OFF:], C, "eps_res")
        return _transformer(nm, h, p.sd, p.p, layers, False, None)

    def lower(prod):
        p = c(prod)
        untouched = [(0, n)] + ([(2 * n, (2 + n_res) * n)] if kind == 2 else [])
        return p.ops, p.weights, p.act, p.shr, {}, B, (lambda a: a[n: 2 * n].view(B, T, C)), untouched, [T * C] * (2 + n_res)
    return Case(site, shape, family, eps, form, lower, ring=True, gn=True, pad_rows=_pad16(B * T), kernel="k_tf128", rows=T)


RES256_SHAPES = [(1, 1, 37, 2, "whole"), (2, 8, 5, 2, "pair8")]                  # (kind, T, B, n_res, form): MDT_OP_RES256


def res256_case(shape, family, eps, B_rows=None):
    import os
    kind, T, B, n_res, form_ = shape
    C, G = 256, 8
    site = "k_res256 GN"
    x, sk = _res_inputs(site, family, kind, B, T, C, G, n_res)
    if B_rows is not None:
        x, sk, B = x[B_rows].contiguous(), (None if sk is None else sk[:, B_rows].contiguous()), len(B_rows)
    blocks = [f"res{k}." for k in range(n_res)]
    built = {}

    def c(prod):
        if prod not in built:
            old = os.environ.get("MDT_RES256")
            os.environ["MDT_RES256"] = "1"               # (read when a compiler is made: test_gpu_ops.test_resnet_chain_256 sets it too)
            try:
                built[prod] = oc.resnet_chain256(kind, T, B, n_res, form_, prod or "f32", x=x, sk=sk,
                                                 sd_edit=_mid(blocks, family))
            finally:
                if old is None:
                    del os.environ["MDT_RES256"]
                else:
                    os.environ["MDT_RES256"] = old
            built[prod].ops[0].f[rt.FF_EPS_RES] = eps["eps_res"]
        return built[prod]
    n = B * T * C

    def form(nm):
        p = c(None)
        return _res_chain(nm, x, sk, p.sd, blocks, kind, G, p.shr[oc.FILM_OFF:], C, "eps_res")

    def lower(prod):
        p = c(prod)
        untouched = [(0, n)] + ([(2 * n, (2 + n_res) * n)] if kind == 2 else [])
        return p.ops, p.weights, p.act, p.shr, p.ext, B, (lambda a: a[n: 2 * n].view(B, T, C)), untouched, [T * C] * (2 + n_res)
    return Case(site, shape, family, eps, form, lower, ring=True, gn=True, pad_rows=_pad16(B * T), kernel="k_res256", rows=T)


# ---- the list of cases ------------------------------------------------------------------------------------------------------------
# (id, builder, args): every case the GPU test runs, built on demand (a case holds its tensors; nothing is kept past the next).

def _all():
    out = []

    def add(fn, *args, fams=FAMILIES, eps):
        for fam in fams:
            for ev in eps_variants(eps):
                out.append((fn, args + (fam, ev)))
    for s in GN_SHAPES:
        for what in ("mean", "rstd"):
            for fam in FAMILIES:
                for ev in eps_variants({"eps": GN_PROD_EPS[s]}):
                    out.append((gn_stats_case, (s, fam, ev, what)))
        add(gemm_gn_case, s, eps={"eps": GN_PROD_EPS[s]})
    for s in LN_GEMM_SHAPES:
        add(gemm_ln_case, s, eps={"eps": 1e-5})
    for s in SPLIT_SHAPES:
        for pro in (rt.PRO_LAYERNORM, rt.PRO_GROUPNORM):
            for fam in FAMILIES:
                for ev in eps_variants({"eps": 1e-5}):
                    out.append((split_gemm_case, (s, fam, ev, pro)))
    for s in GN_ACT_SHAPES:
        add(gn_act_case, s, eps={"eps": s[6]})
    for s in GN_ACT2_SHAPES:
        add(gn_act2_case, s, eps={"eps": 1e-5})
    for s in PROJ_SHAPES:
        add(proj_case, s, eps={"eps": 1e-5})
    for s in RCONV_SHAPES:
        add(rconv_case, s, eps={"eps": 1e-5})
    for s in RCONV2_SHAPES:
        add(rconv2_case, s, eps={"eps": 1e-5})
    for s in RESBLOCK_SHAPES:
        add(resblock_case, s, fams=RESBLOCK_FAMILIES, eps={"eps": 1e-5})
    for s in TBLOCK_SHAPES:
        for mode in tblock_modes(s[1], s[3]):
            add(tblock_case, s, mode, eps={"eps_ln": 1e-5})
    for s in TF_SHAPES:
        add(tf_case, s, fams=TF_FAMILIES, eps=TF_EPS)
    for s in RES128_SHAPES:
        add(res128_case, s, fams=RES_FAMILIES, eps=RES128_EPS)
    for s in RES256_SHAPES:
        add(res256_case, s, fams=RES_FAMILIES, eps={"eps_res": 1e-5})
    return out


CASES = _all()


def case_id(entry):
    fn, args = entry
    parts = []
    for a in args:
        if isinstance(a, dict):
            parts.append(",".join(f"{v:g}" for v in a.values()))
        elif isinstance(a, tuple):
            parts.append("(" + ",".join(str(v) for v in a) + ")")
        else:
            parts.append(str(a))
    return fn.__name__[: -len("_case")] + "-" + "-".join(parts)


@functools.lru_cache(maxsize=2)
def _build(index):
    fn, args = CASES[index]
    return fn(*args)


def build(entry):
    return _build(CASES.index(entry))
