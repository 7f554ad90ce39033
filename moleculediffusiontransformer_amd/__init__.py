"""MI355X-native inverse-diffusion sampling path of MoleculeDiffusionTransformer.

Drop-in classes (same names and call signatures as the reference's MoleculeDiffusion package):

    from moleculediffusiontransformer_amd import QMDiffusion, QMDiffusionForward

The sampling hot path (QMDiffusion.sample -> ADPM2 sampler -> 1-D conditional U-Net) runs in
hand-written gfx950 kernels (csrc/, C ABI in include/mdt_hip.h).  So does the VALUE of the training objective,
``model.eval_loss(sequences, output, device)`` (one noise level per sample, no gradients); ``forward()`` itself stays PyTorch.
"""
from .diffusion import (ADPM2Sampler, AEulerSampler, DiffusionInpainter, DiffusionSampler, KarrasSampler,  # noqa: F401
                        KarrasSchedule, LogNormalDistribution, NoiseSource, Sampler, guidance_rows, refine_start)
from .generative import (DESCRIPTOR_NAMES, DescriptorLimits, KDiffusion_mod, KnownSet, QMDiffusion, QMDiffusionForward, Screened, SmilesVocabulary, SubstructureSet,  # noqa: F401
                         XDiffusion_x, complete_and_validate, edit_distance, formula_strings, generate_and_validate, guidance_sweep,
                         has_substructure, has_substructure_normalized, mol_fingerprint, mol_descriptors, mol_formula, mol_graph, mol_hydrogens, mol_key, mol_normalize, mol_rings, mol_weight, nearest_known, nearest_known_tanimoto, one_hot_draft, predict_properties_from_tokens, refine_and_validate, screen_candidates,
                         mol_canon, mol_respell, mol_same, mol_scaffold, mol_write, scaffold_keep, scaffold_key, scaffold_tokens, screen_tokens,
                         screen_tokens_diverse, smiles_check, strength_sweep, tanimoto, tokens_to_forward_input,
                         SubstructureCounts, substructure_keep, substructure_map,
                         McsResult, mcs_keep, mcs_tokens, mol_difference, mol_mcs)
from .graphmodel import AnalogDiffusionFull, AnalogDiffusionSparse  # noqa: F401
from .modules import PositionalEncoding1D, UNetCFG1d  # noqa: F401
from .netspec import UNetConfig, forward_unet_config, inverse_unet_config  # noqa: F401

__version__ = "0.1.0"


def count_parameters(model) -> None:
    """utils.py:16-25 of the reference."""
    total = sum(p.numel() for p in model.parameters())
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    print("-" * 100)
    print("Total parameters: ", total, " trainable parameters: ", trainable)
    print("-" * 100)
