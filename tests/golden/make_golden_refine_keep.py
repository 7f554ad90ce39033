"""Fixtures for refine_keep(keep_mask=) / refine_keep_tokens(keep_mask=) from the REAL reference (build container only):

    python tests/golden/make_golden_refine_keep.py

Built on make_golden_refine.py's recipe (reference imported at generation time only, synthetic weights, NoiseInjector draws, data
only).  The reference has both halves -- the noising line and the merge of its inpaint loop (diffusion.py:535-542, :549) and the
sampler's step() -- but no function that joins them.  For the duration of ONE m.sample(...) call the sampler class's forward() is
replaced by

    x = src + sigmas[k] * noise
    for i in range(k, num_steps - 1):
        x = where(mask, src + sigmas[i] * randn_like(src), x)
        x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1])
    return where(mask, src, x)

where ``noise`` is the call's own first draw (generative.py:853).  The NoiseInjector's counter is set to T + i in front of the source
draw of step i and to i + 1 in front of the step: the entry is ``<tag>/draw0``, step i takes ``<tag>/draw{i + 1}`` and its source draw
``<tag>/draw{T + i}``, whatever the start -- a row's result depends on its own start only, so the per-sample case (rows) is stitched
from scalar runs, as in make_golden_refine.py.

  refine_keep.npz   per case <c>: <c>_seq, <c>_draft (B, L) int64, <c>_keep (B, L) bool, <c>_start (B,) int64, <c>_out (B, C, L),
                    <c>_tokens (B, L) int64, <c>_timesteps, <c>_cond_scale, <c>_margin (B,) (the smallest top-two margin of each row);
                    cases = their names, models = the synthetic model of each, samplers = 'adpm2' | 'aeuler', masks = the mask of
                    each, tags = the noise tag; free_tokens_changed = the free tokens that differ from the draft, over the cases

The generator asserts on the CPU that (a) an all-False mask is make_golden_refine.refine() bit for bit, (b) the kept positions of
every output equal the source exactly, (c) EVERY position of every case has a top-two margin above MARGIN (twice the 1e-4 sample
tolerance of the GPU tests: no position is left out of a token comparison; if that fails on a rebuild, move the case's start or
mask), and (d) over the cases at least one free token differs from the draft.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (imports the reference)
import make_golden_inpaint_tokens as IT  # noqa: E402
import make_golden_refine as RF  # noqa: E402

import MoleculeDiffusion.generative as RG  # type: ignore  # noqa: E402

MARGIN = IT.MARGIN   # twice the 1e-4 sample tolerance of the GPU tests
B, T, L = 3, 8, 32


def masks():
    """(B, L) keep masks.  'mix': kept and free positions in every row -- an aligned block, every third position (changes inside
    every group of four), a block that starts and ends inside a group.  'edge': one row fully kept, one fully free, one mixed."""
    mix = torch.zeros(B, L, dtype=torch.bool)
    mix[0, :12] = True
    mix[1, ::3] = True
    mix[2, 5:19] = True
    edge = torch.zeros(B, L, dtype=torch.bool)
    edge[0] = True
    edge[2, 1::2] = True
    edge[2, 24:] = True
    return {"mix": mix, "edge": edge}


#        case    model   sampler   cond_scale  start       mask
CASES = [("a", "tiny", "adpm2", 1.0, 4, "mix"),
         ("b", "tiny", "adpm2", 2.0, 1, "edge"),
         ("c", "pd22", "adpm2", 2.0, 3, "mix"),
         ("d", "pd22", "aeuler", 2.0, 0, "edge"),
         ("e", "tiny", "aeuler", 2.0, 2, "mix"),
         ("f", "pd22", "aeuler", 1.0, 1, "edge"),
         ("g", "pd22", "adpm2", 1.0, 0, "edge"),
         ("rows", "tiny", "adpm2", 2.0, [1, 3, 5], "mix")]


def refine_keep(m, seq, src, mask, k, cond_scale, sampler_name, tag, timesteps=T):
    """The reference's m.sample() with the sampler's forward() replaced by the loop of the module docstring."""
    sampler = RF.make_sampler(sampler_name)
    cls = type(sampler)
    inj = G.NoiseInjector(tag)
    orig_forward, orig_name = cls.forward, RG.ADPM2Sampler

    def forward(self, noise, fn, sigmas, num_steps):
        assert inj.n == 1 and num_steps == timesteps       # the call's first draw has been made (generative.py:853)
        x = src + sigmas[k] * noise
        for i in range(k, num_steps - 1):
            inj.n = num_steps + i
            x = torch.where(mask, src + sigmas[i] * torch.randn_like(src), x)
            inj.n = i + 1
            x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1])
        return torch.where(mask, src, x)
    cls.forward = forward
    RG.ADPM2Sampler = lambda rho: sampler
    try:
        with inj, torch.no_grad():
            out = m.sample(seq, "cpu", cond_scale=cond_scale, timesteps=timesteps, clamp=False)
    finally:
        cls.forward, RG.ADPM2Sampler = orig_forward, orig_name
    assert inj.n == timesteps, (tag, inj.n)                # the last step took draw T - 1
    return out


def case(name, m, model, C, sampler, cond_scale, start, keep):
    seq, draft, _ = IT.inputs(B, C, L)
    src = IT.one_hot(draft, C)
    mask = keep.unsqueeze(1).repeat(1, C, 1)
    tag = f"rk_{model}"
    starts = [start] * B if isinstance(start, int) else list(start)
    runs = {k: refine_keep(m, seq, src, mask, k, cond_scale, sampler, tag) for k in sorted(set(starts))}
    out = torch.stack([runs[k][b] for b, k in enumerate(starts)])       # row b from the scalar run at start[b]
    tokens = torch.argmax(torch.permute(out, (0, 2, 1)), dim=2)
    assert torch.equal(out[mask], src[mask]) and torch.equal(tokens[keep], draft[keep]), name                  # (b)
    mg = RF.margins(out)
    changed = int((tokens != draft)[~keep].sum())
    print(f"case {name}: starts {starts}, smallest top-two margin per row {[f'{float(v):.2e}' for v in mg]}, "
          f"free tokens changed {changed} of {int((~keep).sum())}")
    assert float(mg.min()) > MARGIN, (name, mg)                                                                # (c)
    return changed, {f"{name}_seq": seq, f"{name}_draft": draft, f"{name}_keep": keep, f"{name}_start": np.array(starts, dtype=np.int64),
                     f"{name}_out": out, f"{name}_tokens": tokens, f"{name}_timesteps": T, f"{name}_cond_scale": cond_scale,
                     f"{name}_margin": mg}


def identities(m, model, C):
    """(a): with nothing kept the loop is make_golden_refine.refine(), bit for bit."""
    seq, draft, _ = IT.inputs(B, C, L)
    src = IT.one_hot(draft, C)
    none = torch.zeros(B, C, L, dtype=torch.bool)
    for sampler in ("adpm2", "aeuler"):
        for k, cs in ((0, 1.0), (3, 2.0), (T - 2, 1.0)):
            want = RF.refine(m, seq, src, k, cs, sampler, f"rk_{model}")
            assert torch.equal(refine_keep(m, seq, src, none, k, cs, sampler, f"rk_{model}"), want), (model, sampler, k)
    print(f"an all-False mask is the unmasked refine for {model}")


def main():
    torch.set_num_threads(8)
    built, rows, changed = {}, {}, 0
    mk = masks()
    for name, model, sampler, cs, start, mask in CASES:
        kw = IT.MODELS[model]
        assert kw["max_length"] == L
        if model not in built:
            built[model] = G.build("inverse", context_embedding_max_length=12, text_embed_dim=64, embed_dim_position=64, **kw)
            identities(built[model], model, kw["pred_dim"])
        n, arrs = case(name, built[model], model, kw["pred_dim"], sampler, cs, start, mk[mask])
        changed += n
        rows.update(arrs)
    assert changed > 0                                                                                          # (d)
    rows["free_tokens_changed"] = changed
    rows["cases"] = np.array([c[0] for c in CASES])
    rows["models"] = np.array([c[1] for c in CASES])
    rows["samplers"] = np.array([c[2] for c in CASES])
    rows["masks"] = np.array([c[5] for c in CASES])
    rows["tags"] = np.array([f"rk_{c[1]}" for c in CASES])
    G.save("refine_keep.npz", **rows)


if __name__ == "__main__":
    main()
