"""Fixtures for inpaint_tokens() from the REAL reference (build container only):

    python tests/golden/make_golden_inpaint_tokens.py

Same recipe as make_golden.py (reference imported at generation time only, synthetic weights, NoiseInjector draws in the
reference's call order, data only).  Every case is the reference's own model.inpaint on what inpaint_from_draft_and_conditioning
hands it (generative.py:1600-1614): the +-1 one-hot of the draft ids, permuted to (B, C, L), the (B, L) mask repeated over the
channels; the tokens are its permute + argmax of the result.

  inpaint_tokens.npz    per case <c> in a, b, c: <c>_seq, <c>_draft (B, L) int64, <c>_keep (B, L) bool, <c>_out (B, C, L),
                        <c>_tokens (B, L) int64, <c>_ndraws, <c>_timesteps, <c>_num_resamples, <c>_cond_scale, <c>_margin (the
                        smallest top-two margin of the result over the generated positions); cases = their names, models = the
                        synthetic model of each, tags = the noise tag of each

The GPU path is held to 1e-4 on the sample, so a token can be asked to match wherever the reference's top-two margin exceeds 2e-4:
the generator asserts that EVERY generated position of every case does (no position is left out of the token check), that the kept
region is the one-hot draft bit for bit, that kept tokens are the draft's, and the draw count 1 + (T - 1) * 2R.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (imports the reference)
from moleculediffusiontransformer_amd.synth import synth_normal  # noqa: E402

MARGIN = 2e-4        # twice the 1e-4 sample tolerance of the GPU tests

#        case  model   B  T  R  cond_scale  noise tag
CASES = [("a", "tiny", 3, 6, 2, 2.0, "it_tiny_a"),
         ("b", "tiny", 3, 8, 1, 1.0, "it_tiny_b"),
         ("c", "pd22", 2, 6, 3, 2.0, "it_pd22")]
MODELS = {"tiny": dict(max_length=32, pred_dim=16, channels=16), "pd22": dict(max_length=32, pred_dim=22, channels=32)}


def inputs(B, C, L):
    seq = synth_normal("tiny/seq", (3, 12))[:B]
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(7))
    keep = torch.zeros(B, L, dtype=torch.bool)
    keep[0, :12] = True
    keep[1, ::3] = True
    if B == 3:
        keep[2, 20:] = True
    return seq, draft, keep


def one_hot(draft, C):
    """encode_SMILES_into_one_hot's tensor half (generative.py:1567-1569) and the permute of :1603."""
    oh = F.one_hot(draft.long(), num_classes=C)
    oh[oh == 0] = -1
    return torch.permute(oh.float(), (0, 2, 1))


def case(name, m, C, L, B, T, R, cond_scale, tag):
    seq, draft, keep = inputs(B, C, L)
    src = one_hot(draft, C)
    mask = keep.unsqueeze(1).repeat(1, C, 1)                       # repeat(in_paint_mask, 'b l -> b p l', p=num_classes), :1600
    inj = G.NoiseInjector(tag)
    with inj, torch.no_grad():
        out = m.inpaint(seq, "cpu", cond_scale=cond_scale, timesteps=T, num_resamples=R, inpaint=src, in_paint_mask=mask)
    tokens = torch.argmax(torch.permute(out, (0, 2, 1)), dim=2)    # :1613-1614
    assert inj.n == 1 + (T - 1) * 2 * R, (name, inj.n)
    assert torch.equal(out[mask], src[mask]), name
    assert torch.equal(tokens[keep], draft[keep]), name
    top2 = torch.topk(out, 2, dim=1).values
    margin = float((top2[:, 0] - top2[:, 1])[~keep].min())
    assert margin > MARGIN, (name, margin)
    print(f"case {name}: {inj.n} draws, smallest top-two margin at a generated position {margin:.3e}")
    return {f"{name}_seq": seq, f"{name}_draft": draft, f"{name}_keep": keep, f"{name}_out": out, f"{name}_tokens": tokens,
            f"{name}_ndraws": inj.n, f"{name}_timesteps": T, f"{name}_num_resamples": R, f"{name}_cond_scale": cond_scale,
            f"{name}_margin": margin}


def main():
    torch.set_num_threads(8)
    built, rows = {}, {}
    for name, model, B, T, R, cs, tag in CASES:
        kw = MODELS[model]
        if model not in built:
            built[model] = G.build("inverse", context_embedding_max_length=12, text_embed_dim=64, embed_dim_position=64, **kw)
        rows.update(case(name, built[model], kw["pred_dim"], kw["max_length"], B, T, R, cs, tag))
    rows["cases"] = np.array([c[0] for c in CASES])
    rows["models"] = np.array([c[1] for c in CASES])
    rows["tags"] = np.array([c[6] for c in CASES])
    G.save("inpaint_tokens.npz", **rows)


if __name__ == "__main__":
    main()
