"""High-precision restatements of the small kernels' operations, shared by
test_ops_direct_gpu.py / test_grad_prims_gpu.py and checked on the CPU by test_direct_refs_cpu.py.
Plain torch on the CPU; nothing here touches the GPU or the native library."""
import functools
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                                                  # f32 unit roundoff
# one rounding of a 16-bit output (half an ulp, doubled), relative
OUT_ROUND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


# ------------------------------------------------------------------ sine position embedding
def sine_dim_t(num_pos_feats, temperature=10000):
    """The modules' own f32 expression (kinet_amd/models/position_encoding.py)."""
    k = torch.arange(num_pos_feats, dtype=torch.float32)
    return temperature ** (2 * (k // 2) / num_pos_feats)


def sine_embed_ref(mask, num_pos_feats, three_d=False, frame=0, frames=1, normalize=True, scale=2 * math.pi,
                   level_embed=None, dtype=torch.float64):
    """mask (B, H, W) bool -> (B, H*W, C) rows, channel order [z|]y|x, sin (even) / cos (odd).
      2-d: e = (cumsum - 0.5) / (last + 1e-6) * scale     3-d: e = cumsum / (last + 1e-6) * scale,
      z = the cumsum over the frames axis of the mask repeated per frame, taken at `frame`."""
    B, H, W = mask.shape
    valid = (~mask).to(dtype)
    y, x = valid.cumsum(1), valid.cumsum(2)
    ytot, xtot = y[:, -1:, :], x[:, :, -1:]
    parts = []
    if three_d:
        z, ztot = valid * (frame + 1), valid * frames
        if normalize:
            z, y, x = (e / (t + 1e-6) * scale for e, t in ((z, ztot), (y, ytot), (x, xtot)))
        parts = [z, y, x]
    else:
        if normalize:
            y, x = ((e - 0.5) / (t + 1e-6) * scale for e, t in ((y, ytot), (x, xtot)))
        parts = [y, x]
    dim_t = sine_dim_t(num_pos_feats).to(dtype)
    odd = (torch.arange(num_pos_feats) % 2).bool()
    out = []
    for e in parts:
        a = e[..., None] / dim_t
        out.append(torch.where(odd, a.cos(), a.sin()))
    out = torch.cat(out, -1).reshape(B, H * W, -1)
    if level_embed is not None:
        out = out + level_embed.to(dtype)
    return out


def sine_compared(mask, num_pos_feats, three_d, normalize):
    """(B, H*W, C) bool: the positions a test compares.  In the 2-d normalised case a row
    without a valid pixel makes the x argument -0.5 / 1e-6 * 2pi ~ -3e6 (likewise a column and y):
    sin / cos of that is ill-conditioned in the reference itself; those (pixel, axis) pairs are
    excluded, everything else is compared."""
    B, H, W = mask.shape
    C = (3 if three_d else 2) * num_pos_feats
    keep = torch.ones(B, H, W, C, dtype=torch.bool)
    if normalize and not three_d:
        col_ok = (~mask).any(1)            # (B, W): y channels
        row_ok = (~mask).any(2)            # (B, H): x channels
        keep[..., :num_pos_feats] = col_ok[:, None, :, None]
        keep[..., num_pos_feats:] = row_ok[:, :, None, None]
    return keep.reshape(B, H * W, C)


def sine_excluded_share(mask):
    """Per image: the share of (pixel, axis) pairs excluded in 2-d normalised mode."""
    keep = sine_compared(mask, 1, False, True)           # one channel per axis
    return 1.0 - keep.float().mean((1, 2))


def main_masks():
    """B=3, H=11, W=17: unmasked / 9x13 valid (right + bottom padding) / interior holes plus one
    fully masked row and column."""
    m = torch.zeros(3, 11, 17, dtype=torch.bool)
    m[1, 9:, :] = True
    m[1, :, 13:] = True
    m[2] = torch.rand(11, 17, generator=torch.Generator().manual_seed(0)) < 0.3
    m[2, 4, :] = True
    m[2, :, 6] = True
    return m


def sine_geometries():
    """name -> mask.  The small ones cover the 4-lane split with H or W < 4, a block tail, a pixel
    count that is a multiple of 64, and one fully masked image."""
    g = torch.Generator().manual_seed(1)
    geo = {'main': main_masks()}
    geo['1x1'] = torch.zeros(1, 1, 1, dtype=torch.bool)
    m = torch.zeros(2, 3, 2, dtype=torch.bool)
    m[1, 0, 1] = True
    geo['3x2'] = m
    m = torch.zeros(1, 2, 70, dtype=torch.bool)
    m[:, :, 60:] = True
    m[0, 1, 7] = True
    geo['2x70'] = m
    m = torch.zeros(1, 70, 3, dtype=torch.bool)
    m[:, 60:, :] = True
    m[0, 33, 1] = True
    geo['70x3'] = m
    m = torch.zeros(2, 8, 8, dtype=torch.bool)
    m[1, 6:, :] = True
    m[1, :, 7:] = True
    geo['8x8'] = m
    m = torch.rand(2, 5, 6, generator=g) < 0.25
    m[0, :, 0] = False                     # image 0: holes only, every row / column keeps a pixel
    m[0, 2, :] = False
    m[1] = True                            # image 1: fully masked
    geo['allmasked'] = m
    return geo


FULLY_MASKED = {('allmasked', 1)}          # exempt from the 25 % cap (all of it is excluded in 2-d normalised mode)


# ------------------------------------------------------------------------------ box refine
def inverse_sigmoid_ref(x, eps=1e-5):
    x = x.double().clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


SPECIAL_REFS = [0.0, 1.0, 1e-7, 1 - 1e-7, -1e-3, 1.001, 0.5, 1e-5, 1 - 1e-5]


def box_case(B, Q, L, rd):
    """Seeded inputs of one box_refine case: tmp (B, Q, 4), ref (B, Q, rd), valid_ratios (B, L, 2)."""
    g = torch.Generator().manual_seed(B * 1000 + Q * 10 + L + rd)
    tmp = torch.rand(B, Q, 4, generator=g) * 16 - 8
    ref = torch.rand(B, Q, rd, generator=g)
    # the clamp points, spread over every column and over positive and negative tmp
    flat = ref.view(-1)
    n = min(flat.numel(), 4 * len(SPECIAL_REFS))
    flat[:n] = torch.tensor(SPECIAL_REFS * 4)[:n]
    if Q > 8:
        tmp.view(-1)[::37] = 30.0
        tmp.view(-1)[5::41] = -30.0
        tmp[:, :4, :rd] = torch.tensor([7.0, -7.0, 3.0, -3.0])[:, None]     # special refs with both signs of tmp
    # distinct per batch, level and axis (a shuffled grid of spacing 0.6 / (2 B L) >= 0.025), so a
    # wrong b or l index, or x / y swapped, shows
    nv = B * L * 2
    vr = (0.3 + 0.6 * (torch.randperm(nv, generator=g) + 0.5) / nv).view(B, L, 2)
    return tmp, ref, vr


def box_refine_ref(tmp, ref, valid_ratios=None):
    """f64, from the f32 inputs: new = sigmoid(tmp + pad4(inverse_sigmoid(ref))),
    ref_input = new[:, :, None] * cat([vr, vr], -1)[:, None]."""
    t = tmp.double().clone()
    rd = ref.shape[-1]
    t[..., :rd] += inverse_sigmoid_ref(ref)
    new = torch.sigmoid(t)
    if valid_ratios is None:
        return new, None
    vr = valid_ratios.double()
    return new, new[:, :, None] * torch.cat([vr, vr], -1)[:, None]


# ------------------------------------------------------------------------------ layernorm
def layernorm_ref(x, gamma, beta, eps=1e-5, residual=None):
    """f64 layer norm of the inputs as given (already rounded to the tested dtype); x + residual
    is formed in f64."""
    v = x.double()
    if residual is not None:
        v = v + residual.double()
    return F.layer_norm(v, (x.shape[-1],), gamma.double(), beta.double(), eps)


def layernorm_vec_eligible(dtype, d):
    """Row length on which kinet_layernorm takes the 16-byte vector kernel (aligned pointers)."""
    es = 4 if dtype == torch.float32 else 2
    return (d * es) % 16 == 0 and d * es <= 1024


# ------------------------------------------------------------------------ im2col / col2im
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(H, W, KH, KW, stride, pad):
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    return (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1


def unfold_nhwc(x, KH, KW, stride, pad):
    """x (B, H, W, C) -> (B*Ho*Wo, KH*KW*C): F.unfold on the NCHW view, its (c, kh, kw) row order
    permuted to the kernel's (kh, kw, c)."""
    B, H, W, C = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2), (KH, KW), padding=_pair(pad), stride=_pair(stride))   # (B, C*KH*KW, L)
    L = u.shape[-1]
    return u.view(B, C, KH, KW, L).permute(0, 4, 2, 3, 1).reshape(B * L, KH * KW * C)


def fold_nhwc(cols, x_shape, KH, KW, stride, pad):
    """The adjoint: cols (B*Ho*Wo, KH*KW*C) -> (B, H, W, C) through F.fold."""
    B, H, W, C = x_shape
    L = cols.shape[0] // B
    u = cols.view(B, L, KH, KW, C).permute(0, 4, 2, 3, 1).reshape(B, C * KH * KW, L)
    return F.fold(u, (H, W), (KH, KW), padding=_pair(pad), stride=_pair(stride)).permute(0, 2, 3, 1).contiguous()


def unfold_naive(x, KH, KW, stride, pad):
    B, H, W, C = x.shape
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    Ho, Wo = out_size(H, W, KH, KW, stride, pad)
    cols = torch.zeros(B * Ho * Wo, KH * KW * C, dtype=x.dtype)
    for n in range(B):
        for ho in range(Ho):
            for wo in range(Wo):
                for kh in range(KH):
                    for kw in range(KW):
                        h, w = ho * sh - ph + kh, wo * sw - pw + kw
                        if 0 <= h < H and 0 <= w < W:
                            t = kh * KW + kw
                            cols[(n * Ho + ho) * Wo + wo, t * C:(t + 1) * C] = x[n, h, w]
    return cols


def fold_naive(cols, x_shape, KH, KW, stride, pad):
    B, H, W, C = x_shape
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    Ho, Wo = out_size(H, W, KH, KW, stride, pad)
    dx = torch.zeros(B, H, W, C, dtype=cols.dtype)
    for n in range(B):
        for ho in range(Ho):
            for wo in range(Wo):
                for kh in range(KH):
                    for kw in range(KW):
                        h, w = ho * sh - ph + kh, wo * sw - pw + kw
                        if 0 <= h < H and 0 <= w < W:
                            t = kh * KW + kw
                            dx[n, h, w] += cols[(n * Ho + ho) * Wo + wo, t * C:(t + 1) * C]
    return dx


# --------------------------------------------------------------------------------- gemm_tn
def tn_exact_bound(a64, b64):
    """Exact paths (f32 MFMA = an fma chain; products of 16-bit operands are exact in f32): the
    standard worst case of any summation order of K terms, gamma_K ~ K u, on |a|^T |b|; +64 for the
    split-K finalize (at most 64 slices summed in f32)."""
    K = a64.shape[0]
    return 1.01 * (K + 64) * U32 * (a64.abs().T @ b64.abs()) + 1e-30


@functools.lru_cache(maxsize=None)
def tn_operands(K, M, N, dtype, seed=0):
    """Seeded operands rounded to `dtype`, with the f64 product of the rounded values."""
    g = torch.Generator().manual_seed(seed + K * 131 + M * 17 + N)
    a = torch.randn(K, M, generator=g).to(dtype)
    b = torch.randn(K, N, generator=g).to(dtype)
    return a, b, a.double().T @ b.double()
