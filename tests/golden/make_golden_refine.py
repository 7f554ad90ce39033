"""Fixtures for refine() / refine_tokens() from the REAL reference (build container only):

    python tests/golden/make_golden_refine.py

Same recipe as make_golden_inpaint_tokens.py (reference imported at generation time only, synthetic weights, NoiseInjector draws,
data only).  The reference has no refine function, but it has the arithmetic: ``x = src + sigmas[k] * randn_like(src)`` is the
noising line of its inpaint loop (diffusion.py:535-539) and the sampler's step() is unchanged.  For the duration of ONE
m.sample(...) call the sampler class's forward() is replaced by

    x = src + sigmas[k] * noise
    for i in range(k, num_steps - 1): x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1])

where ``noise`` is the call's own first draw (generative.py:853), and the NoiseInjector's counter is set to k + 1 after that draw:
step i takes the ABSOLUTE draw ``<tag>/draw{i + 1}``, whatever the start.  A row's result then depends on its own start only,
which is what makes the per-sample cases (rows*) legitimate: row b is taken from the scalar run at start[b].

  refine.npz    per case <c>: <c>_seq, <c>_draft (B, L) int64, <c>_start (B,) int64, <c>_out (B, C, L), <c>_tokens (B, L) int64,
                <c>_timesteps, <c>_cond_scale, <c>_margin (B,) (the smallest top-two margin of each row of the result);
                cases = their names, models = the synthetic model of each, samplers = 'adpm2' | 'aeuler', tags = the noise tag

The GPU path is held to 1e-4 on the sample, so a token can be asked to match wherever the reference's top-two margin exceeds 2e-4:
the generator asserts that EVERY position of every case does.  If that fails on a rebuild, move the case to a neighbouring start.
It also asserts, on the CPU, that a zero source at start 0 is m.sample() bit for bit, and that KarrasSampler() without churn
returns src + sigmas[k] * draw0 bit for bit (the reference's degenerate correction line, diffusion.py:434).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (imports the reference)
import make_golden_inpaint_tokens as IT  # noqa: E402
from moleculediffusiontransformer_amd.synth import synth_normal  # noqa: E402

import MoleculeDiffusion.diffusion as RD  # type: ignore  # noqa: E402
import MoleculeDiffusion.generative as RG  # type: ignore  # noqa: E402

MARGIN = IT.MARGIN   # twice the 1e-4 sample tolerance of the GPU tests
B, T = 3, 8

#        case     model   sampler   cond_scale  start
CASES = [("a", "tiny", "adpm2", 1.0, 4),
         ("b", "tiny", "adpm2", 2.0, 3),
         ("c", "pd22", "adpm2", 1.0, 4),
         ("d", "pd22", "adpm2", 2.0, 3),
         ("e", "tiny", "aeuler", 2.0, 2),
         ("f", "pd22", "aeuler", 1.0, 5),
         ("rows1", "tiny", "adpm2", 2.0, [1, 3, 5]),
         ("rows2", "pd22", "adpm2", 1.0, [0, 4, 6])]


def make_sampler(name):
    return {"adpm2": lambda: RD.ADPM2Sampler(rho=1), "aeuler": RD.AEulerSampler, "karras": RD.KarrasSampler}[name]()


def refine(m, seq, src, k, cond_scale, sampler_name, tag, timesteps=T):
    """The reference's m.sample() with the sampler's forward() started at step k on the noised source."""
    sampler = make_sampler(sampler_name)
    cls = type(sampler)
    inj = G.NoiseInjector(tag)
    orig_forward, orig_name = cls.forward, RG.ADPM2Sampler

    def forward(self, noise, fn, sigmas, num_steps):
        assert inj.n == 1                                  # the call's first draw has been made (generative.py:853)
        inj.n = k + 1
        x = src + sigmas[k] * noise
        extra = (lambda i: {})
        if sampler_name == "karras":
            gammas = torch.where((sigmas >= self.s_tmin) & (sigmas <= self.s_tmax),
                                 min(self.s_churn / num_steps, 2 ** 0.5 - 1), 0.0)
            extra = (lambda i: dict(gamma=gammas[i]))
        for i in range(k, num_steps - 1):
            x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1], **extra(i))
        return x
    cls.forward = forward
    RG.ADPM2Sampler = lambda rho: sampler
    try:
        with inj, torch.no_grad():
            out = m.sample(seq, "cpu", cond_scale=cond_scale, timesteps=timesteps, clamp=False)
    finally:
        cls.forward, RG.ADPM2Sampler = orig_forward, orig_name
    assert inj.n == timesteps, (tag, inj.n)                # the last step took draw T - 1
    return out


def margins(out):
    top2 = torch.topk(out, 2, dim=1).values
    return (top2[:, 0] - top2[:, 1]).flatten(1).min(dim=1).values


def case(name, m, model, C, L, sampler, cond_scale, start):
    seq, draft, _ = IT.inputs(B, C, L)
    src = IT.one_hot(draft, C)
    tag = f"rf_{model}"
    starts = [start] * B if isinstance(start, int) else list(start)
    runs = {k: refine(m, seq, src, k, cond_scale, sampler, tag) for k in sorted(set(starts))}
    out = torch.stack([runs[k][b] for b, k in enumerate(starts)])       # row b from the scalar run at start[b]
    tokens = torch.argmax(torch.permute(out, (0, 2, 1)), dim=2)
    mg = margins(out)
    assert float(mg.min()) > MARGIN, (name, mg)
    print(f"case {name}: starts {starts}, smallest top-two margin per row {[f'{float(v):.2e}' for v in mg]}, "
          f"tokens changed {int((tokens != draft).sum())} of {tokens.numel()}")
    return {f"{name}_seq": seq, f"{name}_draft": draft, f"{name}_start": np.array(starts, dtype=np.int64), f"{name}_out": out,
            f"{name}_tokens": tokens, f"{name}_timesteps": T, f"{name}_cond_scale": cond_scale, f"{name}_margin": mg}


def identities(m, model, C, L):
    seq, draft, _ = IT.inputs(B, C, L)
    src = IT.one_hot(draft, C)
    for sampler, tag in (("adpm2", f"rf_{model}"), ("aeuler", f"rf_{model}")):
        inj = G.NoiseInjector(tag)
        smp, orig = make_sampler(sampler), RG.ADPM2Sampler
        RG.ADPM2Sampler = lambda rho: smp
        try:
            with inj, torch.no_grad():
                full = m.sample(seq, "cpu", cond_scale=1.0, timesteps=T, clamp=False)
        finally:
            RG.ADPM2Sampler = orig
        assert torch.equal(refine(m, seq, torch.zeros_like(src), 0, 1.0, sampler, tag), full), (model, sampler)
    sig = RD.KarrasSchedule(sigma_min=0.001, sigma_max=9.0, rho=3.0)(T, "cpu")
    for k in (0, 3, T - 2):
        out = refine(m, seq, src, k, 1.0, "karras", f"rf_{model}")
        assert torch.equal(out, src + sig[k] * synth_normal(f"rf_{model}/draw0", tuple(src.shape))), (model, k)
    print(f"identities hold for {model}")


def main():
    torch.set_num_threads(8)
    built, rows = {}, {}
    for name, model, sampler, cs, start in CASES:
        kw = IT.MODELS[model]
        if model not in built:
            built[model] = G.build("inverse", context_embedding_max_length=12, text_embed_dim=64, embed_dim_position=64, **kw)
            identities(built[model], model, kw["pred_dim"], kw["max_length"])
        rows.update(case(name, built[model], model, kw["pred_dim"], kw["max_length"], sampler, cs, start))
    # the known answer of the GPU suite: at the last start the reference keeps every token of the draft
    kw = IT.MODELS["tiny"]
    seq, draft, _ = IT.inputs(B, kw["pred_dim"], kw["max_length"])
    last = refine(built["tiny"], seq, IT.one_hot(draft, kw["pred_dim"]), T - 2, 1.0, "adpm2", "rf_tiny")
    assert torch.equal(torch.argmax(last, dim=1), draft)
    rows["last_start_margin"] = float(margins(last).min())
    print(f"start {T - 2} on tiny keeps all {draft.numel()} tokens, margin {rows['last_start_margin']:.3e}")
    rows["cases"] = np.array([c[0] for c in CASES])
    rows["models"] = np.array([c[1] for c in CASES])
    rows["samplers"] = np.array([c[2] for c in CASES])
    rows["tags"] = np.array([f"rf_{c[1]}" for c in CASES])
    G.save("refine.npz", **rows)


if __name__ == "__main__":
    main()
