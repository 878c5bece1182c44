"""Cases of the ViT-Adapter backbone fixture (tests/golden/vit_adapter.npz): model settings, image sizes and the synthesis of
images and parameters from the counter hash of msda_cases.py, shared by tools/make_vit_adapter_golden.py (which runs the
reference on them) and the tests.  Nothing is stored but results.

Training-mode cases carry a ``tag``: ReLU and max-pool make the gradients discontinuous, so the generator searches tags
"t0", "t1", ... in order until every ReLU pre-activation and every pool window of the reference's run clears RELU_MARGIN /
POOL_MARGIN (relative to the tensor's largest magnitude, in float64 and in float32), and stores the tag it settled on.
"""
from __future__ import annotations

import numpy as np

import msda_cases as mc

RELU_MARGIN = 1e-5          # |pre-activation| >= RELU_MARGIN * max |pre-activation| of its tensor
POOL_MARGIN = 1e-5          # a pool window's winner leads the runner-up by POOL_MARGIN * max |input| of the pool
MAX_TAGS = 64

# SpatialPriorModule, eval mode with non-trivial running statistics; "odd" has H / 32 = 3
SPM_EVAL = {
    "odd": dict(inplanes=16, embed_dim=64, B=2, H=96, W=128),
    "even": dict(inplanes=32, embed_dim=96, B=1, H=128, W=160),
}
SPM_TRAIN = dict(inplanes=16, embed_dim=64, B=2, H=32, W=64)

# a reduced ViTAdapter every kernel accepts: two interactions (the last with extra extractors), block 0 windowed
BACKBONE = dict(pretrain_size=64, embed_dim=192, depth=4, num_heads=3, mlp_ratio=4, conv_inplane=16, n_points=4, deform_num_heads=6,
                init_values=0.5, cffn_ratio=0.25, deform_ratio=0.5, interaction_indexes=[[0, 1], [2, 3]], drop_path_rate=0.0,
                window_attn=[True, False, False, False], window_size=[14, None, None, None])
BACKBONE_EVAL = dict(B=1, H=256, W=320)         # H / 16 = 16 > 14: the windowed block pads
BACKBONE_TRAIN = dict(B=2, H=32, W=64)
# parameters of the backbone/train case whose gradients are stored (prefix match), besides the image gradient
BACKBONE_TRAIN_GRADS = ("level_embed", "pos_embed", "up.", "norm1.", "norm2.", "norm3.", "norm4.", "spm.", "interactions.0.")
# ... except these two: a per-channel constant added straight ahead of a training-mode batch norm (f1 = norm1(up(c2) + fc1(..) + x1))
# shifts the batch mean and nothing else, so its gradient is exactly zero; the reference's float64 run returns rounding noise
# there, which has no scale to compare against.  The generator asserts the noise level, the test the product's.
BACKBONE_TRAIN_ZERO_GRADS = ("up.bias", "spm.fc1.bias")

# the Base detection recipe (configs/mask_rcnn/mask_rcnn_meta_transformer_adapter_base_fpn_3x_coco.py:9-29), minus `pretrained`
DET_BASE = dict(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, drop_path_rate=0.3, conv_inplane=64, n_points=4,
                deform_num_heads=12, cffn_ratio=0.25, deform_ratio=0.5, interaction_indexes=[[0, 2], [3, 5], [6, 8], [9, 11]],
                window_attn=[True, True, False, True, True, False, True, True, False, True, True, False],
                window_size=[14, 14, None, 14, 14, None, 14, 14, None, 14, 14, None])


def image(case: str, tag: str, B: int, H: int, W: int) -> np.ndarray:
    """[B, 3, H, W] in [-2, 2) on a 2^-9 grid (a normalised RGB batch by magnitude)"""
    return mc.uniform((B, 3, H, W), mc.seed_of("vit_adapter", case, tag, "image"), -2.0, 2.0, bits=11)


def cotangent(case: str, tag: str, name: str, shape) -> np.ndarray:
    return mc.uniform(tuple(shape), mc.seed_of("vit_adapter", case, tag, "d" + name))


def state_dict_arrays(keys_shapes, tag: str) -> dict:
    """msda_cases.state_dict_arrays, with the batch-norm modules (those with a running_mean) and the position table given
    values of their kind: weight around 1, running_mean in [-0.25, 0.25), running_var in [0.5, 1.5), a zero step count"""
    keys_shapes = [(k, tuple(s)) for k, s in keys_shapes]
    bn = {k[: -len("running_mean")] for k, _ in keys_shapes if k.endswith("running_mean")}
    plain = [(k, s) for k, s in keys_shapes if not any(k.startswith(p) for p in bn) and k != "pos_embed"]
    out = mc.state_dict_arrays(plain, tag)
    for k, s in keys_shapes:
        if k in out:
            continue
        seed = mc.seed_of(tag, k)
        if k == "pos_embed":
            a = mc.uniform(s, seed, -0.25, 0.25)
        elif k.endswith("num_batches_tracked"):
            out[k] = np.zeros(s, dtype=np.int64)
            continue
        elif k.endswith("running_mean"):
            a = mc.uniform(s, seed, -0.25, 0.25)
        elif k.endswith("running_var"):
            a = mc.uniform(s, seed, 0.5, 1.5)
        elif k.endswith("weight"):
            a = 1.0 + mc.uniform(s, seed, -0.125, 0.125)
        else:
            a = mc.uniform(s, seed, -0.0625, 0.0625)
        out[k] = a.astype(np.float16).astype(np.float32)
    return {k: out[k] for k, _ in keys_shapes}


def tags():
    return [f"t{i}" for i in range(MAX_TAGS)]
