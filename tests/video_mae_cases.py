"""Cases, input builders and float64 restatements for the VideoMAE pre-training tests (a plain module, like hyperspectral_cases.py).

Restated from the formulas, not from the code under test:
  * the tubelet gather and the token order (Video/models/modeling_finetune.py:277-297: Conv3d with kernel = stride, then
    ``flatten(2).transpose(1, 2)``: token n = (t', h', w') row-major; a row of the flattened weight runs (c, dt, dh, dw));
  * the index lists (boolean indexing keeps ascending positions) and the assembly of modeling_pretrain.py:349-356;
  * the target and the loss of Video/engine_for_pretraining.py:75-105: ``u = x std + mean``; per token and channel over the
    p0 p1 p2 pixels of the patch the mean and the UNBIASED variance, ``label = (u - mean) / (sqrt(var) + 1e-6)``, columns
    ``(p0 p1 p2 c)``; ``l = mean_cols (pred - label)^2``; ``loss = sum(w l) / sum(w)`` with ``w = mask[decoded positions]``;
  * the model around the Blocks (modeling_pretrain.py:124-139, 223-236, 340-360), with oracle.block_oracle for the Blocks.
tests/test_video_mae_cpu.py ties them to einops and to the reference-made fixture tests/golden/video_mae.npz."""
from __future__ import annotations

import zlib

import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)        # timm.data.constants.IMAGENET_DEFAULT_MEAN / _STD (engine_for_pretraining.py:68-74)
STD = (0.229, 0.224, 0.225)

# the model of every fixture case (the issue's sizes)
MODEL = dict(enc_dim=32, enc_heads=2, enc_depth=2, dec_dim=32, dec_heads=2, dec_depth=1, eps=1e-6, B=2, tubelet=2, in_chans=3)
CASES = {"p16": dict(img=32, patch=16, frames=4, masked=6),        # 2 x 2 x 2 = 8 tokens, 2 visible
         "p8": dict(img=24, patch=8, frames=6, masked=21)}         # 3 x 3 x 3 = 27 tokens, 6 visible; 8-pixel lines, 128 pixels per patch
# variant -> (case, with a decoder mask, init_values)
VARIANTS = {"p16": ("p16", False, 0.), "p16_dm": ("p16", True, 0.), "p8": ("p8", False, 0.), "p8_dm": ("p8", True, 0.),
            "p8_ls_dm": ("p8", True, 0.1)}
# gradients the fixture holds.  The tubelet projection's is as large as the weight (196 KB at p16): the fixture has to stay under 1 MB, so
# it is stored whole for the variants with a decoder mask (the ones whose cal_loss_mask has a zero) and as the output channels
# PROJ_GRAD_ROWS (`<v>/grad_rows/...`, every column of those filters) for the others.
GRAD_KEYS = ("mask_token", "encoder_to_decoder.weight", "encoder.blocks.1.attn.proj.weight")
GRAD_KEYS_DM = GRAD_KEYS + ("encoder.patch_embed.proj.weight",)


PROJ_GRAD_ROWS = (0, 16)


def grad_keys(variant: str):
    return GRAD_KEYS_DM if VARIANTS[variant][1] else GRAD_KEYS


def _seed(tag: str) -> int:
    return zlib.crc32(tag.encode()) & 0x7FFFFFFF


def n_tokens(case: str) -> int:
    c = CASES[case]
    return (c["frames"] // MODEL["tubelet"]) * (c["img"] // c["patch"]) ** 2


def tubelet(case: str):
    return (MODEL["tubelet"], CASES[case]["patch"], CASES[case]["patch"])


def model_kwargs(case: str, init_values: float = 0.) -> dict:
    """constructor arguments of PretrainVisionTransformer (the reference's and this package's alike; norm_layer is added by the caller)"""
    c, m = CASES[case], MODEL
    return dict(img_size=c["img"], patch_size=c["patch"], encoder_in_chans=m["in_chans"], encoder_embed_dim=m["enc_dim"],
                encoder_depth=m["enc_depth"], encoder_num_heads=m["enc_heads"], decoder_num_classes=m["in_chans"] * m["tubelet"] * c["patch"] ** 2,
                decoder_embed_dim=m["dec_dim"], decoder_depth=m["dec_depth"], decoder_num_heads=m["dec_heads"], qkv_bias=True,
                init_values=init_values, tubelet_size=m["tubelet"], all_frames=c["frames"])


# ------------------------------------------------------------------------------------------------------------------ inputs

def make_clip(case: str, B: int = MODEL["B"]) -> np.ndarray:
    """a normalised clip [B, 3, T, H, W] float32 (what the data loader hands over), values on a 1/64 grid"""
    c = CASES[case]
    rng = np.random.default_rng(_seed("clip/" + case))
    return (np.round(rng.standard_normal((B, MODEL["in_chans"], c["frames"], c["img"], c["img"])) * 64) / 64).astype(np.float32)


def make_masks(case: str, B: int = MODEL["B"]):
    """(mask, decode_mask) bool [B, N]: `masked` random positions per sample; the decoder mask keeps every second masked position plus
    one visible position DECODED, i.e. those are its False entries (the decoded positions are ~decode_mask), so cal_loss_mask has a zero"""
    N, masked = n_tokens(case), CASES[case]["masked"]
    rng = np.random.default_rng(_seed("mask/" + case))
    mask, dmask = np.zeros((B, N), dtype=bool), np.ones((B, N), dtype=bool)
    for b in range(B):
        pos = np.sort(rng.permutation(N)[:masked])
        mask[b, pos] = True
        dmask[b, pos[::2]] = False
        dmask[b, rng.choice(np.flatnonzero(~mask[b]))] = False
    return mask, dmask


def low_contrast_clip(case: str, B: int = MODEL["B"]) -> np.ndarray:
    """make_clip with ONE low-contrast patch: token 1 of sample 0 holds 0.3 + 1e-3 * normal noise (spread 1e-3 around 0.3) in every channel.
    There eps on the standard deviation, eps on the variance and no eps give different labels; a constant patch would not do (the
    reference's own fp32 result is rounding noise there)."""
    x = make_clip(case, B)
    kt, kh, kw = tubelet(case)
    Wp = CASES[case]["img"] // kw
    hp, wp = 1 // Wp, 1 % Wp                                              # token 1: t' = 0
    rng = np.random.default_rng(_seed("low/" + case))
    x[0, :, 0:kt, hp * kh:(hp + 1) * kh, wp * kw:(wp + 1) * kw] = (0.3 + 1e-3 * rng.standard_normal((MODEL["in_chans"], kt, kh, kw))).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------------------------ restatements

def sinusoid_table(n: int, d: int) -> torch.Tensor:
    """get_sinusoid_encoding_table (modeling_finetune.py:302-318): float64 arithmetic, float32 table [n, d]"""
    pos, j = np.arange(n, dtype=np.float64)[:, None], np.arange(d)[None, :]
    t = pos / np.power(10000.0, 2 * (j // 2) / d)
    t[:, 0::2], t[:, 1::2] = np.sin(t[:, 0::2]), np.cos(t[:, 1::2])
    return torch.from_numpy(t.astype(np.float32))


def index_list(sel) -> torch.Tensor:
    """True positions of a bool [B, N] selection, ascending per sample -> int64 [B, n] (what boolean indexing + reshape(B, -1) keeps)"""
    sel = np.asarray(sel)
    rows = [np.flatnonzero(r) for r in sel]
    assert len({len(r) for r in rows}) == 1, "unequal counts"
    return torch.from_numpy(np.stack(rows).astype(np.int64))


def index_lists(mask, decode_mask=None):
    """(vis_idx, dec_idx, w): visible = ~mask; decoded = mask, or ~decode_mask when given; w = mask[decoded] as float64"""
    mask = np.asarray(mask)
    dec = mask if decode_mask is None else ~np.asarray(decode_mask)
    vis_idx, dec_idx = index_list(~mask), index_list(dec)
    w = torch.from_numpy(np.take_along_axis(mask, dec_idx.numpy(), axis=1).astype(np.float64))
    return vis_idx, dec_idx, w


def gather_restate(video: torch.Tensor, idx: torch.Tensor, kt: int, kh: int, kw: int) -> torch.Tensor:
    """[B, n, C kt kh kw] in the video's dtype: row (b, j) = the tubelet of token idx[b, j], columns (c, dt, dh, dw)"""
    B, C, T, H, W = video.shape
    Hp, Wp = H // kh, W // kw
    out = video.new_empty(B, idx.shape[1], C * kt * kh * kw)
    for b in range(B):
        for j, n in enumerate(idx[b].tolist()):
            tp, hp, wp = n // (Hp * Wp), (n // Wp) % Hp, n % Wp
            out[b, j] = video[b, :, tp * kt:(tp + 1) * kt, hp * kh:(hp + 1) * kh, wp * kw:(wp + 1) * kw].reshape(-1)
    return out


def labels_restate(video: torch.Tensor, kt: int, kh: int, kw: int, normalize: bool = True, eps_mode: str = "std", mean=MEAN, std=STD,
                   dtype=torch.float64) -> torch.Tensor:
    """the target of EVERY token, [B, N, kt kh kw C] in `dtype`.  eps_mode: "std" is the reference's (sqrt(var) + 1e-6); "var"
    (sqrt(var + 1e-6)) and "none" are the two mistakes the low-contrast patch tells apart."""
    B, C, T, H, W = video.shape
    m = torch.tensor(mean, dtype=dtype).view(1, C, 1, 1, 1)
    s = torch.tensor(std, dtype=dtype).view(1, C, 1, 1, 1)
    u = video.to(dtype) * s + m
    Tp, Hp, Wp = T // kt, H // kh, W // kw
    u = u[:, :, :Tp * kt, :Hp * kh, :Wp * kw].reshape(B, C, Tp, kt, Hp, kh, Wp, kw).permute(0, 2, 4, 6, 3, 5, 7, 1)
    u = u.reshape(B, Tp * Hp * Wp, kt * kh * kw, C)
    if normalize:
        n = u.shape[2]
        mu = u.sum(dim=2, keepdim=True) / n
        var = ((u - mu) ** 2).sum(dim=2, keepdim=True) / (n - 1)
        den = {"std": var.sqrt() + 1e-6, "var": (var + 1e-6).sqrt(), "none": var.sqrt()}[eps_mode]
        u = (u - mu) / den
    return u.reshape(B, Tp * Hp * Wp, -1)


def take(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x [B, N, C] (or [N, C]) rows idx [B, n] -> [B, n, C]"""
    if x.dim() == 2:
        return x[idx]
    return torch.gather(x, 1, idx.unsqueeze(-1).expand(-1, -1, x.shape[-1]))


def loss_restate(pred: torch.Tensor, labels: torch.Tensor, w: torch.Tensor, g: float = 1.0):
    """(loss, per-token losses [B, Ndec], dpred) in float64; sum(w) = 0 -> loss 0 and a zero gradient"""
    pred, labels, w = pred.double(), labels.double(), w.double()
    d = pred - labels
    tok = (d ** 2).mean(dim=-1)
    sw = w.sum()
    if float(sw) == 0.0:
        return torch.zeros((), dtype=torch.float64), tok, torch.zeros_like(d)
    return (tok * w).sum() / sw, tok, g * 2.0 * w.unsqueeze(-1) * d / (d.shape[-1] * sw)


def assemble_restate(xv: torch.Tensor, pos: torch.Tensor, vis_idx, dec_idx, mask_token: torch.Tensor) -> torch.Tensor:
    """cat(xv + pos[vis_idx], mask_token + pos[dec_idx]) (modeling_pretrain.py:349-356); pos [N, Cd], mask_token [Cd]"""
    B = xv.shape[0]
    return torch.cat([xv + pos[vis_idx], (mask_token + pos[dec_idx]).expand(B, -1, -1)], dim=1)


def _block_params(sd: dict, prefix: str) -> dict:
    p = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    q, v = p.pop("attn.q_bias"), p.pop("attn.v_bias")
    p["attn.qkv.bias"] = torch.cat([q, torch.zeros_like(v), v])             # modeling_finetune.py:172-178
    return p


def model_restate(sd: dict, case: str, clip: torch.Tensor, mask, decode_mask=None, dtype=torch.float64, encoder_only: bool = False):
    """PretrainVisionTransformer.forward on a reference state dict `sd` (reference keys), in `dtype`"""
    from oracle import block_oracle as bo
    m = MODEL
    sd = {k: v.to(dtype) for k, v in sd.items()}
    kt, kh, kw = tubelet(case)
    N = n_tokens(case)
    vis_idx, dec_idx, _ = index_lists(mask, decode_mask)

    def blocks(x, side, depth, heads):
        for i in range(depth):
            p = _block_params(sd, f"{side}.blocks.{i}.")
            x = bo.block_forward(x, p, heads, eps=m["eps"], gamma1=p.get("gamma_1"), gamma2=p.get("gamma_2"), pre_scale_q=True)
        return bo.layer_norm(x, sd[f"{side}.norm.weight"], sd[f"{side}.norm.bias"], m["eps"]) if side == "encoder" else x

    w = sd["encoder.patch_embed.proj.weight"]
    rows = gather_restate(clip.to(dtype), vis_idx, kt, kh, kw)
    x = rows @ w.reshape(w.shape[0], -1).t() + sd["encoder.patch_embed.proj.bias"] + sinusoid_table(N, m["enc_dim"]).to(dtype)[vis_idx]
    x = blocks(x, "encoder", m["enc_depth"], m["enc_heads"])
    if encoder_only:
        return x
    x = x @ sd["encoder_to_decoder.weight"].t()
    x = assemble_restate(x, sinusoid_table(N, m["dec_dim"]).to(dtype), vis_idx, dec_idx, sd["mask_token"].reshape(-1))
    x = blocks(x, "decoder", m["dec_depth"], m["dec_heads"])
    if dec_idx.shape[1] > 0:
        x = x[:, -dec_idx.shape[1]:]
    x = bo.layer_norm(x, sd["decoder.norm.weight"], sd["decoder.norm.bias"], m["eps"])
    return x @ sd["decoder.head.weight"].t() + sd["decoder.head.bias"]


def fixture_state_dict(gold, variant: str) -> dict:
    """the reference state dict of a fixture variant: the case's weights, plus the layer-scale vectors of a `_ls` variant"""
    case = VARIANTS[variant][0]
    sd = {k[len(case) + 4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(case + "/sd/")}
    if VARIANTS[variant][2] > 0:
        sd.update({k[len(case) + 7:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(case + "/sd_ls/")})
    return sd
