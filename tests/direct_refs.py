"""High-precision restatements of the small kernels' operations, shared by
test_ops_direct_gpu.py / test_grad_prims_gpu.py / test_grad_norm_attn_gpu.py /
test_train_ops_direct_gpu.py / test_gemm_tiles_direct_gpu.py / test_msda_direct_gpu.py / test_attn_direct_gpu.py /
test_stem_conv3x3_direct_gpu.py and checked on the CPU by test_direct_refs_cpu.py.
Plain torch on the CPU; nothing here touches the GPU or the native library."""
import functools
import math

import numpy as np
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


# =================================================== training path: csrc/grad.hip, csrc/train_ops.hip
# Bounds are per element: bound_i = c * U32 * A_i (+ OUT_ROUND * |ref_i| for a 16-bit output), A_i the
# reference's formula on absolute values (the running-error majorant), c the length of the longest
# sequential f32 chain an element passes through, derived beside each constant below.
F32_TINY = 2.0 ** -126                                            # below it f32 results lose bits / flush


def eps32(eps):
    """The launchers take eps as a float: the f64 references use the same rounded value."""
    return float(np.float32(eps))


# ------------------------------------------------------------------------ dropout hash
def dropout_thresh_ref(p):
    """uint32(double(float32(p)) * 2^24 + 0.5): p is rounded to f32 first (0.1 -> 1677721)."""
    t = float(np.float32(p)) * 16777216.0 + 0.5
    return 16777216 if t >= 16777216.0 else (0 if t <= 0.0 else int(t))


def dropout_keep_ref(seed, idx, p):
    """The keep decision of common.h's dropout_keep restated in numpy uint64 (wraparound):
    z = seed + idx * golden; two xor-shift-multiply rounds of the splitmix64 finaliser; z ^= z >> 31;
    kept iff the top 24 bits >= thresh.  seed is an int64 (negative seeds wrap), idx any shape."""
    s = np.array([seed], dtype=np.int64).astype(np.uint64)
    z = s + np.atleast_1d(np.asarray(idx)).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)) >= np.uint64(dropout_thresh_ref(p))


def dropout_seed_for_draw(draw, idx, low=0x5A5A5A5A5A):
    """The int64 seed for which element idx's 24-bit uniform draw is exactly `draw` (every step of
    the hash is a bijection mod 2^64, inverted here in Python integers): a seed that sits on the
    threshold, or one below it, at a chosen element."""
    m = (1 << 64) - 1
    z = ((draw << 40) | low) & m
    z = z ^ (z >> 31) ^ (z >> 62)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & m
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & m
    z = z ^ (z >> 30) ^ (z >> 60)
    s = (z - idx * 0x9E3779B97F4A7C15) & m
    return s - (1 << 64) if s >= (1 << 63) else s


def keep_mask(seed, shape, p):
    """bool tensor of `shape`: element with row-major flat index i is kept iff dropout_keep_ref(seed, i, p).
    LayerNorm (rows, d): i = r*d + c.  Attention (B, H, Lq, Lk): i = ((b*H + h)*Lq + i)*Lk + j."""
    n = int(np.prod(shape))
    return torch.from_numpy(dropout_keep_ref(seed, np.arange(n, dtype=np.uint64), p)).view(*shape)


def keep_scale64(p):
    """1 / (1 - p) of the f32-rounded p, in f64 (the kernels round it once more: 2 u, inside c)."""
    return 1.0 / (1.0 - float(np.float32(p)))


def keep_scale32(p):
    """The kernels' own f32 value 1.f / (1.f - p)."""
    return float(np.float32(1) / (np.float32(1) - np.float32(p)))


# ------------------------------------------------------------------------------ colsum
def colsum_chunks(rows):
    """kinet_colsum_workspace's row chunking: (chunks, rows per chunk)."""
    chunks = max(1, min(256, rows // 64))
    return chunks, (rows + chunks - 1) // chunks if rows else 0


def colsum_c(rows):
    """An element passes through at most rc - 1 adds of its chunk's serial loop (the vector kernel's
    chain is shorter), 1 add of the final kernel's per-thread loop (<= 256 chunks: one each) and the
    8 levels of its LDS tree."""
    return colsum_chunks(rows)[1] + 8


# ------------------------------------------------------------------- LayerNorm backward
def ln_c(d, rows_chain):
    """Chains of the one-wave-per-row LayerNorm kernels (forward and backward, both files), nv =
    ceil(d / 64) values per lane, every reduction nv adds + 6 shuffle levels:
      xh = (z - mean) * rstd: mean nv + 6 adds + 1 divide; + 1 subtraction; rstd half the relative
           error of the variance (nv + 6 adds, 1 square, 1 divide, 1 + eps: (nv + 9) / 2) + 2 for
           rsqrtf; + 1 product                                          -> 1.5 nv + 15.5
      dx = rstd * (g - sg/d - xh * sgx/d): xh; the outer rstd (nv + 9) / 2 + 2; sgx = sum g xh:
           nv + 6 adds + 2 products; 1/d and its product 2; xh * .: 1; 2 subtractions, the outer
           product, g = dy gamma: 4                                     -> 3 nv + 37
      dgamma = sum_r dy xh: xh + 1 product + the row chain;  dbeta: the row chain,
    rows_chain = rows per wave (serial) + 4 waves + 1 + 8 (final per-thread loop and tree)."""
    nv = (d + 63) // 64
    return {'xh': 1.5 * nv + 16, 'dx': 3 * nv + 37, 'dg': 1.5 * nv + 17 + rows_chain, 'db': rows_chain}


def ln_ref(z, gamma, beta, eps, dy=None, zA=None):
    """f64 LayerNorm of the rows z (rows, d), its closed-form backward for dy, and the majorants.
    zA: |z|'s majorant where z is itself a sum (x + r Z s)."""
    z, gamma = z.double(), gamma.double()
    zA = z.abs() if zA is None else zA
    mean = z.mean(-1, keepdim=True)
    rstd = (((z - mean) ** 2).mean(-1, keepdim=True) + eps32(eps)).rsqrt()
    xh = (z - mean) * rstd
    xhA = (zA + zA.mean(-1, keepdim=True)) * rstd
    out = {'xh': xh, 'xhA': xhA, 'rstd': rstd}
    if beta is not None:
        out['y'] = xh * gamma + beta.double()
        out['yA'] = xhA * gamma.abs() + beta.double().abs()
    if dy is not None:
        dy = dy.double()
        g = dy * gamma
        gA = g.abs()
        out['dz'] = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        out['dzA'] = rstd * (gA + gA.mean(-1, keepdim=True) + xhA * (gA * xhA).mean(-1, keepdim=True))
        out['dg'], out['dgA'] = (dy * xh).sum(0), (dy.abs() * xhA).sum(0)
        out['db'], out['dbA'] = dy.sum(0), dy.abs().sum(0)
    return out


@functools.lru_cache(maxsize=None)
def ln_case(rows, d, dtype, seed=0, offset=0.0):
    """Seeded LayerNorm-backward inputs rounded to `dtype` (gamma f32)."""
    g = torch.Generator().manual_seed(seed + rows * 1031 + d)
    x = (offset + torch.randn(rows, d, generator=g)).to(dtype)
    dy = torch.randn(rows, d, generator=g).to(dtype)
    gamma = torch.rand(d, generator=g) + 0.5
    beta = torch.randn(d, generator=g)
    return x, dy, gamma, beta


# ------------------------------------------------------------------- GroupNorm backward
def gn_blocks(HW):
    """The launcher's HW blocking: (blocks per image, rows per block)."""
    nb = max(1, min(512, HW // 128))
    return nb, (HW + nb - 1) // nb


def gn_pivot(X):
    """X (N, HW, G, cg) -> (N, 1, G, 1): the kernels' pivot of every (image, group)."""
    return X[:, :4, :, :min(X.shape[-1], 8)].mean((1, 3), keepdim=True)


R_PIVOT = 2.0 ** -24          # x - pivot and pivot + mean_s each round once at the data's own magnitude


def gn_bwd_ref(dy, x, gamma, G, eps):
    """f64 GroupNorm backward on (N, HW, C) NHWC, with majorants and per-element c.  The kernels sum
    x, x^2, dy, dy x per channel (rb rows of a block serially -- the scalar kernel; then nb / 4 + 3
    adds over the blocks), then cg channels per group serially with one gamma product:
    n = rb + nb/4 + 3 + cg + 2 roundings on every group sum.  The sums are of s = x - pivot, the
    pivot the mean of the group's first min(cg, 8) channels at the first min(HW, 4) pixels (gn_pivot).  The
    variance is the one-pass E[s^2] - mean_s^2: its relative error is (n + 3) kappa u, kappa =
    (E[s^2] + mean_s^2) / (var + eps) evaluated in f64 per group (a few units whatever the data's
    offset); rstd takes half of it, + 2 for rsqrtf.
      dx = rstd (g - a/cnt - xh bx/cnt), xh = (x - mean) rstd, bx = rstd (bs - mean a): three factors
           rstd 1.5 (n + 3) kappa + 6; mean n + 1; bs and mean a: 2 n + 4; 8 single operations
                                                                       -> (1.5 kappa + 3) (n + 8)
      dgamma_c = sum_n rstd (sum dy x - mean sum dy): the channel sums rb + nb/4 + 3, mean n + 1,
           rstd 0.5 (n + 3) kappa + 2, 3 operations, N images           -> below
      dbeta_c: rb + nb/4 + 3 + N."""
    N, HW, C = x.shape
    cg = C // G
    X, DY = x.double().view(N, HW, G, cg), dy.double().view(N, HW, G, cg)
    gm = gamma.double().view(1, 1, G, cg)
    ax = (1, 3)
    mean = X.mean(ax, keepdim=True)
    var = ((X - mean) ** 2).mean(ax, keepdim=True)
    e = eps32(eps)
    rstd = (var + e).rsqrt()
    Sx = X - gn_pivot(X)
    kappa = ((Sx * Sx).mean(ax, keepdim=True) + Sx.mean(ax, keepdim=True) ** 2) / (var + e)
    xh = (X - mean) * rstd
    g = DY * gm
    gA = g.abs()
    SA = Sx.abs() + R_PIVOT * X.abs()              # |x - pivot| and the rounding of forming it
    meanA = SA.mean(ax, keepdim=True)
    xhA = (SA + meanA) * rstd
    bxA = rstd * ((gA * SA).mean(ax, keepdim=True) + meanA * gA.mean(ax, keepdim=True))
    nb, rb = gn_blocks(HW)
    chan = rb + nb // 4 + 3
    n = chan + cg + 2
    out = {
        'dx': (rstd * (g - g.mean(ax, keepdim=True) - xh * (g * xh).mean(ax, keepdim=True))).reshape(N, HW, C),
        'dxA': (rstd * (gA + gA.mean(ax, keepdim=True) + xhA * bxA)).reshape(N, HW, C),
        'dx_c': ((1.5 * kappa + 3) * (n + 8)).expand(N, HW, G, cg).reshape(N, HW, C),
        'dg': (DY * xh).sum((0, 1)).reshape(C),
        'dgA': (rstd * ((DY.abs() * SA).sum(1, keepdim=True) + meanA * DY.abs().sum(1, keepdim=True))).sum((0, 1)).reshape(C),
        'dg_c': (0.5 * (n + 3) * kappa + 2 + n + 1).amax(0).expand(1, G, cg).reshape(C) + chan + 3 + N,
        'db': DY.sum((0, 1)).reshape(C), 'dbA': DY.abs().sum((0, 1)).reshape(C), 'db_c': chan + N,
    }
    return out


@functools.lru_cache(maxsize=None)
def gn_case(N, HW, C, dtype, seed=0, offset=0.0):
    g = torch.Generator().manual_seed(seed + N * 7919 + HW * 131 + C)
    x = (offset + torch.randn(N, HW, C, generator=g)).to(dtype)
    dy = torch.randn(N, HW, C, generator=g).to(dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    return x, dy, gamma


# -------------------------------------------------------------------- GroupNorm forward
def gn_fwd_path(dtype, C, G, aligned=True, y_stride=None, HW=1):
    """Restatement of kinet_groupnorm's dispatch (gn_vec_ok and the straddle condition): 'scalar',
    'vector' or 'straddle'.  V = 16 bytes of `dtype`; the vector kernels need whole vectors per row
    (C % V == 0), groups of at least V channels (a vector reaches at most two groups), C / V <= 256
    (one thread per vector of a row), an output batch stride of whole vectors (y_stride, default
    packed = a multiple of C), 16-byte aligned x and y (`aligned`) and HW * C / V < 2^31; a group
    size that is no multiple of V makes vectors straddle two groups."""
    if dtype == torch.float64:
        return 'scalar'
    V = 4 if dtype == torch.float32 else 8
    y_stride = HW * C if y_stride is None else y_stride
    cg = C // G
    if not (C % V == 0 and cg >= V and C // V <= 256 and y_stride % V == 0 and aligned and HW * (C // V) < 2 ** 31):
        return 'scalar'
    return 'straddle' if cg % V else 'vector'


def gn_fwd_chain(path, dtype, HW, C, G):
    """Serial f32 adds behind one group sum on `path`:
      scalar:   a thread sums one channel over its block's pixels (ppb = 64), then the group's cg
                channel sums serially;
      vector:   a thread sums the V elements of its vector over every nslot-th pixel of the block
                (ppb = 128, nslot = 256 / (C/V) row groups), then nslot * (cg/V) thread sums serially;
      straddle: the same per channel (no V), then nslot * cg channel sums serially;
      finalize: tpo = 256 / (2 G) threads (1 above 256 outputs) each sum every tpo-th block partial,
                then the tpo thread sums serially."""
    V = 4 if dtype == torch.float32 else 8
    cg = C // G
    ppb = 64 if path == 'scalar' else 128
    rows = min(HW, ppb)
    nblk = (HW + ppb - 1) // ppb
    if path == 'scalar':
        block = rows + cg
    else:
        nslot = 256 // (C // V)
        per_thread = (rows + nslot - 1) // nslot
        block = per_thread * V + nslot * (cg // V) if path == 'vector' else per_thread + nslot * cg
    tpo = 256 // (2 * G) if 2 * G <= 256 else 1
    return block + (nblk + tpo - 1) // tpo + tpo


def gn_fwd_ref(x, gamma, beta, G, eps, path):
    """f64 GroupNorm forward on (N, HW, C) NHWC: {'y', 'yA', 'y_c'}, |kernel - y| <= y_c u yA.
    The kernel sums s = x - pivot and s^2 per (image, group) (gn_pivot, the backward's rule) with
    n = gn_fwd_chain + 2 roundings (the square, the division by the count) on either sum, and
      mean = pivot + mean_s, var = E[s^2] - mean_s^2, y = (x - mean) rstd gamma + beta.
    x - mean: mean_s carries n + 1 roundings of its own majorant; forming pivot + mean_s rounds once
      at the data's magnitude |mean|, not the shifted one, and so may x - pivot where the two are
      not within a factor 2: 2 u |mean|, which no count on a shifted majorant covers -- it enters yA
      as 2 |mean| / c, so that c u yA holds exactly 2 u |mean| rstd |gamma| of it; the subtraction 1.
    rstd: the one-pass variance has relative error (n + 3) kappa u, kappa = (E[s^2] + mean_s^2) /
      (var + eps) in f64 per group (a few units whatever the data's offset -- with raw sums it is
      ~ 2 mean^2 / var); rstd takes half, + 2 for rsqrtf.
    The two products and the add of beta: 3.     -> c = n + 2 + 0.5 (n + 3) kappa + 2 + 3."""
    N, HW, C = x.shape
    cg = C // G
    X = x.double().view(N, HW, G, cg)
    gm, bt = gamma.double().view(1, 1, G, cg), beta.double().view(1, 1, G, cg)
    ax = (1, 3)
    mean = X.mean(ax, keepdim=True)
    var = ((X - mean) ** 2).mean(ax, keepdim=True)
    e = eps32(eps)
    rstd = (var + e).rsqrt()
    Sx = X - gn_pivot(X)
    kappa = ((Sx * Sx).mean(ax, keepdim=True) + Sx.mean(ax, keepdim=True) ** 2) / (var + e)
    n = gn_fwd_chain(path, x.dtype, HW, C, G) + 2
    c = n + 7 + 0.5 * (n + 3) * kappa
    SA = Sx.abs()
    A = (SA + SA.mean(ax, keepdim=True) + 2 * mean.abs() / c) * rstd * gm.abs() + bt.abs()
    return {'y': ((X - mean) * rstd * gm + bt).reshape(N, HW, C), 'yA': A.reshape(N, HW, C),
            'y_c': c.expand(N, HW, G, cg).reshape(N, HW, C)}


@functools.lru_cache(maxsize=None)
def gn_fwd_case(N, HW, C, dtype, seed=0, offset=0.0):
    """Seeded GroupNorm-forward inputs: x rounded to `dtype`, gamma and beta f32."""
    g = torch.Generator().manual_seed(seed + N * 7919 + HW * 131 + C)
    x = (offset + torch.randn(N, HW, C, generator=g)).to(dtype)
    return x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)


@functools.lru_cache(maxsize=None)
def gn_fwd_torch_f32(N, HW, C, G, seed, offset):
    """torch's CPU f32 group_norm on gn_fwd_case's f32 inputs, as (N, HW, C): the guards' yardstick."""
    x, gamma, beta = gn_fwd_case(N, HW, C, torch.float32, seed, offset)
    return torch.nn.functional.group_norm(x.permute(0, 2, 1).contiguous(), G, gamma, beta, 1e-5).permute(0, 2, 1)


_F32, _BF16, _F16 = torch.float32, torch.bfloat16, torch.float16
_ALL = (_F32, _BF16, _F16)
# (N, HW, C, G), dtypes, the path expected by reading the launcher.
# scalar: C % V != 0; groups of 3; the ppb = 64 edges with groups of 1; one pixel; 2 G = 320 > 256 (the
# finalize's second `base` pass); 2 G = 256 over 10 blocks of 64 (tpo = 1: the finalize's unrolled 8 and a
# tail of 2).  (1, 1, 8, 2): groups of 4 are one f32 vector each, and half a 16-bit one.
GN_FWD_SCALAR = [((2, 5, 30, 6), _ALL), ((2, 35, 36, 12), _ALL), ((1, 63, 8, 8), _ALL), ((1, 64, 8, 8), _ALL),
                 ((1, 65, 8, 8), _ALL), ((1, 1, 8, 2), (_BF16, _F16)), ((1, 1, 6, 2), _ALL),
                 ((1, 40, 320, 160), _ALL), ((1, 600, 256, 128), _ALL)]
# vector: one pixel; the ppb = 128 edges; the model's shape class; C/V = 256 (one slot) with 2 G = 256
# (tpo = 1); tpo = 1 over 11 blocks (unrolled 8 and a tail of 3); tpo = 128; 34 blocks on tpo = 32 threads
GN_FWD_VECTOR = [((1, 1, 8, 2), (_F32,)), ((2, 127, 32, 4), _ALL), ((2, 128, 32, 4), _ALL), ((2, 129, 32, 4), _ALL),
                 ((3, 273, 256, 32), _ALL), ((1, 300, 1024, 128), (_F32,)), ((1, 1400, 512, 128), (_F32,)),
                 ((1, 40, 8, 1), _ALL), ((1, 4300, 32, 4), _ALL)]
# straddle: the model's class (groups of 9); 2 G = 12 does not divide 256; groups of 9 in 16-bit vectors of
# 8, the split on every position 1..7
GN_FWD_STRADDLE = [((1, 300, 288, 32), _ALL), ((2, 35, 36, 6), (_F32,)), ((1, 129, 72, 8), (_BF16, _F16))]


def gn_fwd_cases(path):
    table = {'scalar': GN_FWD_SCALAR, 'vector': GN_FWD_VECTOR, 'straddle': GN_FWD_STRADDLE}[path]
    return [(s, d) for s, ds in table for d in ds]


GN_GUARD = [(2, 273, 256, 32, 'vector'), (1, 300, 288, 32, 'straddle'), (2, 200, 36, 12, 'scalar')]
GN_GUARD_SEED, GN_GUARD_OFFSET = 3, 30.0


# ------------------------------------------------------- fused LayerNorm epilogues
def ln_epilogue_ref(pre64, gamma, beta, eps):
    """Row-wise f64 LayerNorm of the pre-activation pre64 (rows, d): {'y', 'yA', 'y_c'}.  The fused
    epilogues are two-pass (the mean, then the sum of (v - mean)^2), each reduction at most d serial
    adds however the row is spread over lanes:
      v - mean: the mean d + 1 roundings of mean |v|, the subtraction 1;  rstd: half of the variance's
      d + 3 (the squares are of the already centred values: no cancellation), + 2 for rsqrtf;  the
      two products and the add of beta 3                             -> c = 1.5 d + 9
    on yA = (|v - mean| + mean |v|) rstd |gamma| + |beta|: the mean's error is relative to the row's
    magnitude, so a row of 100 + O(1) has a majorant ~100x its values, as it must."""
    v = pre64.double()
    d = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    rstd = (((v - mean) ** 2).mean(-1, keepdim=True) + eps32(eps)).rsqrt()
    gm, bt = gamma.double(), beta.double()
    return {'y': (v - mean) * rstd * gm + bt,
            'yA': ((v - mean).abs() + v.abs().mean(-1, keepdim=True)) * rstd * gm.abs() + bt.abs(),
            'y_c': 1.5 * d + 9, 'rstd': rstd}


def ln_epilogue_yardstick(pre64, gamma, beta, eps=1e-5):
    """(y64, max error of torch's CPU f32 layer_norm of the f32-rounded pre-activation against it)."""
    y = ln_epilogue_ref(pre64, gamma, beta, eps)['y']
    t = torch.nn.functional.layer_norm(pre64.float(), (pre64.shape[-1],), gamma.float(), beta.float(), eps)
    return y, (t.double() - y).abs().max().item()


# ------------------------------------------------------------------- attention fwd / bwd
def attn_ref(q, k, v, do, heads, scale, key_mask=None, keep=None, p=0.0, dtype=torch.float64):
    """Scaled-dot-product attention and its backward in plain torch ops at `dtype` (f64: the
    reference; f32: torch's own CPU evaluation, the yardstick for the kernels' fast exp).  q, do
    (B, Lq, E), k, v (B, Lk, E); key_mask (B, Lk) bool, True = masked; softmax over the unmasked keys,
    P = 0 on a row without one; keep (B, H, Lq, Lk) bool with probability p of a drop.  Returns
    {o, dq, dk, dv} and, at f64, the majorants {oA, dqA, dkA, dvA}."""
    B, Lq, E = q.shape
    D = E // heads

    def sp(t):
        return t.to(dtype).view(B, -1, heads, D).transpose(1, 2)

    def mg(t):
        return t.transpose(1, 2).reshape(B, -1, E)
    Q, K_, V, dO = sp(q), sp(k), sp(v), sp(do)
    S = Q @ K_.transpose(-1, -2) * scale
    if key_mask is not None:
        S = S.masked_fill(key_mask[:, None, None, :], float('-inf'))
    mx = S.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = (S - mx).exp()
    den = e.sum(-1, keepdim=True)
    P = e / torch.where(den > 0, den, torch.ones_like(den))
    Zs = torch.ones((), dtype=dtype) if keep is None else keep.to(dtype) * keep_scale64(p)
    PZ = P * Zs
    dP = Zs * (dO @ V.transpose(-1, -2))
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    out = {'o': mg(PZ @ V), 'dv': mg(PZ.transpose(-1, -2) @ dO), 'dq': mg(dS @ K_ * scale),
           'dk': mg(dS.transpose(-1, -2) @ Q * scale)}
    if dtype == torch.float64:
        dPA = Zs * (dO.abs() @ V.abs().transpose(-1, -2))
        dSA = P * (dPA + (P * dPA).sum(-1, keepdim=True))
        out.update({'oA': mg(PZ @ V.abs()), 'dvA': mg(PZ.transpose(-1, -2) @ dO.abs()),
                    'dqA': mg(dSA @ K_.abs() * scale), 'dkA': mg(dSA.transpose(-1, -2) @ Q.abs() * scale)})
    return out


def attn_yardstick(ref, f32, names):
    """max over the named tensors and their elements of |torch f32 - f64| / A (A > 0)."""
    worst = 0.0
    for n in names:
        A = ref[n + 'A']
        ok = A > 0
        if ok.any():
            worst = max(worst, ((f32[n].double() - ref[n]).abs()[ok] / A[ok]).max().item())
    return worst


@functools.lru_cache(maxsize=None)
def attn_case(B, heads, D, Lq, Lk, seed=0, qscale=1.0):
    g = torch.Generator().manual_seed(seed + D * 10007 + Lq * 211 + Lk)
    E = heads * D
    q = torch.randn(B, Lq, E, generator=g) * qscale
    k = torch.randn(B, Lk, E, generator=g)
    v = torch.randn(B, Lk, E, generator=g)
    do = torch.randn(B, Lq, E, generator=g)
    return q, k, v, do


# ---------------------------------------------------------------------------- msda_prep
def msda_prep_ref(offlog, refs, shapes, qmask, M, L, P):
    """f64 sampling locations (Nb, Lq, M, L, P, 2) and attention weights (Nb, Lq, M, L, P) from the
    packed row [offsets (m, l, p, xy) | logits (m, l, p)], with majorants and c.
      attw: softmax over the head's L*P logits, 0 on masked queries.  d = logit - max: 1 rounding,
            worth |d| u in the exponent; expf 2; numerator and (every term of) the denominator:
            2 (max|d| + 3); the sum L*P; the divide 1.   Values below F32_TINY lose their bits.
      loc:  2-d refs: ref + off / shapes[l, xy] (x by shapes[l, 0], y by shapes[l, 1], as the
            reference module does): 2.  4-d refs: ref_xy + off / P * ref_wh * 0.5: 4."""
    Nb, Lq = offlog.shape[:2]
    n = M * L * P
    o = offlog[..., :2 * n].double().reshape(Nb, Lq, M, L, P, 2)
    lg = offlog[..., 2 * n:3 * n].double().reshape(Nb, Lq, M, L * P)
    d = lg - lg.amax(-1, keepdim=True)
    e = d.exp()
    a = e / e.sum(-1, keepdim=True)
    if qmask is not None:
        a = a.masked_fill(qmask[:, :, None, None], 0.0)
    attw_c = (2 * (d.abs().amax(-1, keepdim=True) + 3) + L * P + 1).expand_as(a)
    rf = refs.double()
    rd = rf.shape[-1]
    rxy = rf[..., :2][:, :, None, :, None, :]
    if rd == 2:
        div = shapes.double()[None, None, None, :, None, :]
        loc, locA, loc_c = rxy + o / div, rxy.abs() + o.abs() / div, 2
    else:
        rwh = rf[..., 2:][:, :, None, :, None, :]
        loc, locA, loc_c = rxy + o / P * rwh * 0.5, rxy.abs() + (o / P * rwh * 0.5).abs(), 4
    return {'loc': loc, 'locA': locA.expand_as(loc), 'loc_c': loc_c,
            'attw': a.view(Nb, Lq, M, L, P), 'attw_c': attw_c.reshape(Nb, Lq, M, L, P)}


def msda_prep_bwd_ref(gloc, gattw, attw, offlog, refs, shapes, M, L, P):
    """Closed-form f64 gradients for the attention weights `attw` as given (0 rows of masked queries
    pass nothing): d_offlog (Nb, Lq, 3 M L P) in offlog's packing, d_refs (Nb, Lq, L, rd).
      d_logit = a (g - sum g a) over the head's L*P: the sum L*P, 3 operations.
      d_off   = d_loc / shape: 1;  4-d: d_loc * 0.5 * wh / P: 3.
      d_ref   = sum over heads and points of d_loc: M*P;  4-d w, h: of d_loc * 0.5 * (off / P): M*P + 3."""
    Nb, Lq = offlog.shape[:2]
    n = M * L * P
    o = offlog[..., :2 * n].double().reshape(Nb, Lq, M, L, P, 2)
    gl, ga, a = gloc.double(), gattw.double().reshape(Nb, Lq, M, L * P), attw.double().reshape(Nb, Lq, M, L * P)
    dlg = a * (ga - (ga * a).sum(-1, keepdim=True))
    dlgA = a * (ga.abs() + (ga.abs() * a).sum(-1, keepdim=True))
    rf = refs.double()
    rd = rf.shape[-1]
    if rd == 2:
        div = shapes.double()[None, None, None, :, None, :]
        doff, off_c = gl / div, 1
        dref, drefA = gl.sum((2, 4)), gl.abs().sum((2, 4))
        ref_c = torch.full_like(dref, M * P)
    else:
        rwh = rf[..., 2:][:, :, None, :, None, :]
        doff, off_c = gl * 0.5 * rwh / P, 3
        t = gl * 0.5 * (o / P)
        dref = torch.cat([gl.sum((2, 4)), t.sum((2, 4))], -1)
        drefA = torch.cat([gl.abs().sum((2, 4)), t.abs().sum((2, 4))], -1)
        ref_c = torch.cat([torch.full_like(dref[..., :2], M * P), torch.full_like(dref[..., :2], M * P + 3)], -1)
    dol = torch.cat([doff.reshape(Nb, Lq, 2 * n), dlg.reshape(Nb, Lq, n)], -1)
    dolA = torch.cat([doff.abs().reshape(Nb, Lq, 2 * n), dlgA.reshape(Nb, Lq, n)], -1)
    dol_c = torch.cat([torch.full((2 * n,), float(off_c)), torch.full((n,), float(L * P + 3))]).double()
    return {'dol': dol, 'dolA': dolA, 'dol_c': dol_c, 'dref': dref, 'drefA': drefA, 'dref_c': ref_c}


def msda_shapes(L):
    """Non-square level shapes (H != W on every level): dividing x by W instead of shapes[l, 0] shows."""
    return torch.tensor([[3 + 2 * l, 5 + 3 * l] for l in range(L)], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def msda_case(Nb, Lq, M, L, P, rd, pad=0, seed=0, logits='randn'):
    """offlog (Nb, Lq, 3 M L P + pad), refs (Nb, Lq, L, rd), shapes, d_loc, d_attw.  logits: 'randn',
    'pm80' (+-80: the max subtraction, weights down to exp(-160)) or 'equal' (uniform weights)."""
    g = torch.Generator().manual_seed(seed + Nb * 7 + Lq * 1009 + M * 101 + L * 11 + P + rd)
    n = M * L * P
    offlog = torch.randn(Nb, Lq, 3 * n + pad, generator=g)
    offlog[..., :2 * n] *= 3
    if logits == 'pm80':
        offlog[..., 2 * n:3 * n] = torch.where(torch.rand(Nb, Lq, n, generator=g) < 0.5, -80.0, 80.0)
    elif logits == 'equal':
        offlog[..., 2 * n:3 * n] = 1.25
    refs = torch.rand(Nb, Lq, L, rd, generator=g)
    gloc = torch.randn(Nb, Lq, M, L, P, 2, generator=g)
    gattw = torch.randn(Nb, Lq, M, L, P, generator=g)
    return offlog, refs, msda_shapes(L), gloc, gattw


# ---------------------------------------------------------------------- inverse_sigmoid
def inv_sigmoid_inputs():
    """The clamp points of SPECIAL_REFS, values around them, and a dense grid over [-0.1, 1.1]."""
    e = float(np.float32(1e-5))
    pts = SPECIAL_REFS + [e * 0.5, e * 2, 1 - e * 0.5, 1 - e * 2, 0.25, 0.75, -0.0, 2.0, -1.0, 1e-30]
    return torch.cat([torch.tensor(pts, dtype=torch.float32), torch.linspace(-0.1, 1.1, 4001)])


def inv_sigmoid_fwd_bwd_ref(x, dy, eps=1e-5):
    """f64 from the f32 inputs, eps rounded to f32.  y = log(x1 / x2), x1 = max(xc, eps), x2 =
    max(1 - xc, eps), xc = clamp(x, 0, 1); dx through torch's clamp masks (the gradient passes where
    min <= v <= max).  Bounds: y -- the subtraction and the quotient are 2 roundings of the
    logarithm's argument (2 u absolute in y), logf 2 ulp of |y|: c = 4 on A = 1 + |y|.
    dx -- 8 operations, both terms of one sign: c = 8 on A = |dx|."""
    e = eps32(eps)
    xv, g = x.double(), dy.double()
    xc = xv.clamp(0, 1)
    x1, x2 = xc.clamp(min=e), (1 - xc).clamp(min=e)
    y = torch.log(x1 / x2)
    dq = g / (x1 / x2)
    d = torch.where(xc >= e, dq / x2, torch.zeros_like(dq)) + torch.where(1 - xc >= e, dq * x1 / (x2 * x2), torch.zeros_like(dq))
    dx = torch.where((xv >= 0) & (xv <= 1), d, torch.zeros_like(d))
    return y, dx


# ======================================= tiled GEMM / implicit convolution (csrc/gemm.hip)
# Two operand classes.  EXACT: small dyadic values whose every f32 partial sum is exact in any
# order, so the expected output is the f64 result rounded ONCE to the output type and the kernel
# must match it bit for bit -- a dropped, doubled or misplaced K chunk, tap, row or column is a
# hard failure.  GENERIC: randn operands under a per-element running-error bound.
#
# Exact class: x in {-1, -1/2, 0, 1/2, 1}, W in {0, +-1/8, +-1/4}: products are multiples of 1/16
# of magnitude <= 1/4, a sum of K <= 2048 of them is a multiple of 1/16 below 2^9 (13 bits);
# scale in {1/2, 1, 2}, bias multiples of 1/4 in [-1, 1], residual multiples of 1/4 in [-2, 2]:
# acc * scale + bias + res is a multiple of 1/32 below 2^11 (16 bits) -- all exact in f32.
# W is drawn sparse (more zeros the longer K is) so that the sums stay small: a 16-bit output must
# still resolve ONE dropped product (exact_headroom).
_EXACT_ACC_STD = 1.25     # target standard deviation of the accumulators


def x3_bound(a64, b64):
    """KINET_F32_X3 (three bf16 MFMA passes): per-product error <= ~2^-16 |a||b| (hi/lo split of both
    operands, lo*lo dropped), plus f32 accumulation: 4e-5 * (|A| @ |B|) elementwise."""
    return 4e-5 * (a64.abs() @ b64.abs()) + 1e-6


def exact_x(shape, g):
    """Multiples of 1/2 in [-1, 1], uniform over the five values (f32)."""
    return torch.randint(-2, 3, shape, generator=g).float() / 2


def exact_w(shape, K, g):
    """Multiples of 1/8 in [-1/4, 1/4] (f32): +-1/8 with probability q each, +-1/4 with q/4 each;
    var(w) = q/16, var(x) = 1/2, so the accumulator's variance is K q / 32 = _EXACT_ACC_STD^2."""
    q = min(0.2, 32 * _EXACT_ACC_STD ** 2 / K)
    u = torch.rand(shape, generator=g)
    w = torch.zeros(shape)
    for lo, hi, v in ((0, q, 1), (q, 2 * q, -1), (2 * q, 2.25 * q, 2), (2.25 * q, 2.5 * q, -2)):
        w[(u >= lo) & (u < hi)] = v
    return w / 8


def exact_epilogue(N, g):
    """(scale, bias) f32 of length N: scale in {1/2, 1, 2}, bias multiples of 1/4 in [-1, 1]."""
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    bias = torch.randint(-4, 5, (N,), generator=g).float() / 4
    return scale, bias


def exact_res(shape, g):
    """Multiples of 1/4 in [-2, 2] (f32; exact in bf16 and f16 too)."""
    return torch.randint(-8, 9, shape, generator=g).float() / 4


def generic_operands(xshape, wshape, K, dtype, g):
    """randn rounded to the compute type; W scaled by K^-1/2 (f32 tensors holding `dtype` values)."""
    x = torch.randn(xshape, generator=g).to(dtype).float()
    w = (torch.randn(wshape, generator=g) / K ** 0.5).to(dtype).float()
    return x, w


def generic_epilogue(N, g):
    return 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g)


def epilogue64(acc64, scale=None, bias=None, res=None, relu=False, row_mask=None):
    """The kernels' epilogue in f64 on (M, N): relu?(acc * scale + bias + res), masked rows -> 0.
    Returns (value, |acc * scale| + |bias| + |res|) -- the second is the bound's majorant."""
    v = acc64 if scale is None else acc64 * scale.double()
    a = v.abs()
    if bias is not None:
        v, a = v + bias.double(), a + bias.double().abs()
    if res is not None:
        v, a = v + res.double(), a + res.double().abs()
    if relu:
        v = v.clamp(min=0)
    if row_mask is not None:
        v = torch.where(row_mask.reshape(-1, 1), torch.zeros_like(v), v)
    return v, a


def gemm_generic_bound(absprod, K, majorant, ref, out_dtype, scale=None, x3=False):
    """Per-element bound of the tiled kernel's output on generic operands:
      accumulation, any order of K exact products in f32 (gamma_K, +64 for split-K slices):
        1.01 (K + 64) u (|A| @ |B|^T)   [tn_exact_bound for the NT product], or x3_bound for
        KINET_F32_X3 (absprod then is its own bound), carried through |scale|;
      the epilogue's three f32 operations: 4 u (|acc scale| + |bias| + |res|);
      the output rounding: OUT_ROUND[dtype] |ref|."""
    acc = absprod if x3 else 1.01 * (K + 64) * U32 * absprod
    if scale is not None:
        acc = acc * scale.double().abs()
    return acc + 4 * U32 * majorant + OUT_ROUND[out_dtype] * ref.abs() + 1e-30


_MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}


def exact_headroom(pre64, scale, out_dtype):
    """True where one dropped product (1/16 in the accumulator, scale/16 in the output) moves the
    exact-class result by at least one ulp of the output type at that magnitude -- so it cannot
    hide inside the single output rounding.  pre64: the epilogue value before rounding."""
    mag = pre64.abs().clamp(min=2.0 ** -20)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - _MANT[out_dtype])
    step = (torch.ones(pre64.shape[-1], dtype=torch.float64) if scale is None else scale.double().abs()) / 16
    return ulp <= step


def conv64(x_nhwc, w_ohwi, stride, pad):
    """F.conv2d in f64 of NHWC x and (Cout, KH, KW, Cin) weights -> (B*Ho*Wo, Cout)."""
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w_ohwi.double().permute(0, 3, 1, 2), stride=_pair(stride),
                 padding=_pair(pad))
    return y.permute(0, 2, 3, 1).reshape(-1, w_ohwi.shape[0])


# The case tables (shared by the GPU module and the CPU checks of the references).
GEMM_TILES = [(32, 64), (64, 64), (64, 128), (128, 64), (128, 128)]
GEMM_K16 = (8, 56, 64, 72, 136, 200)      # 1, 1, 1, 2, 3, 4 K-steps of 64: tails, odd / even counts
GEMM_K32 = (8, 24, 32, 40, 72, 104)       # the same counts of 32-element steps (f32 / x3)


def gemm_shapes(bm, bn):
    """(M, N) around one tile's edges; the last four: scalar store / load paths, a 15-block grid."""
    return [(1, 4), (bm - 1, bn + 4), (bm, bn), (bm + 1, bn - 4), (2 * bm + 3, 2 * bn + 8), (bm + 1, bn + 1), (5, 3),
            (bm, 2 * bn - 2), (3 * bm - 1, 5 * bn - 4)]


def gemm_table(bm, bn, four_byte):
    """(M, N, K): every shape with two K of the cycle, so each K meets three shapes."""
    ks = GEMM_K32 if four_byte else GEMM_K16
    return [(M, N, ks[(i + j) % 6]) for i, (M, N) in enumerate(gemm_shapes(bm, bn)) for j in (0, 3)]


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, dtype, cls, seed=0):
    """(x (M, K), w (N, K), acc64 (M, N), |x| @ |w|^T) of the exact or the generic class; x, w are f32
    tensors holding values of `dtype`."""
    g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 131 + K + (0 if cls == 'exact' else 5))
    if cls == 'exact':
        x, w = exact_x((M, K), g), exact_w((N, K), K, g)
    else:
        x, w = generic_operands((M, K), (N, K), K, dtype, g)
    xd, wd = x.double(), w.double()
    return x, w, xd @ wd.T, xd.abs() @ wd.abs().T


# name: (KH, KW), (sh, sw), (ph, pw), batch, H, W, Cin, Cout
CONV_CASES = {
    'C1': ((3, 3), (1, 1), (1, 1), 2, 5, 7, 64, 72),       # a tile spanning two images
    'C2': ((3, 3), (2, 2), (1, 1), 1, 9, 6, 128, 64),      # the permuted K-step order (two chunks per tap)
    'C3': ((7, 7), (2, 2), (3, 3), 2, 11, 13, 8, 64),      # non-uniform taps, K = 392 with a tail
    'C4': ((1, 1), (2, 2), (0, 0), 2, 7, 9, 64, 132),      # strided 1x1
    'C5a': ((3, 1), (2, 1), (1, 0), 1, 9, 10, 24, 40),
    'C5b': ((1, 3), (1, 2), (0, 1), 1, 9, 10, 24, 40),
    'C5c': ((7, 1), (2, 1), (3, 0), 1, 9, 10, 24, 40),
    'C6a': ((3, 3), (1, 1), (1, 1), 2, 1, 2, 16, 24),      # image smaller than the filter
    'C6b': ((3, 3), (1, 1), (1, 1), 2, 2, 1, 16, 24),
    'C7': ((3, 3), (1, 1), (2, 2), 1, 4, 5, 16, 24),       # pad wider than the centre tap's reach
    'C7b': ((3, 3), (1, 1), (3, 3), 1, 4, 5, 16, 24),      # ... border windows that are ALL padding
    'C8': ((1, 1), (1, 1), (0, 0), 2, 5, 7, 64, 72),       # the plain-GEMM route (lda = Cin)
}


@functools.lru_cache(maxsize=None)
def conv_case(name, dtype, cls):
    """(x NHWC, w (Cout, KH, KW, Cin), acc64 (M, Cout), |x| * |w|) of the exact or generic class."""
    (KH, KW), stride, pad, B, H, W, Cin, Cout = CONV_CASES[name]
    K = KH * KW * Cin
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 97 + (0 if cls == 'exact' else 5))
    if cls == 'exact':
        x, w = exact_x((B, H, W, Cin), g), exact_w((Cout, KH, KW, Cin), K, g)
    else:
        x, w = generic_operands((B, H, W, Cin), (Cout, KH, KW, Cin), K, dtype, g)
    return x, w, conv64(x, w, stride, pad), conv64(x.abs(), w.abs(), stride, pad)


# ======================================= resident-weight GEMM (csrc/gemm_rw.hip)
# The case table of tests/test_gemm_rw_direct_gpu.py, shared with the CPU checks of its references
# (test_direct_refs_cpu.py).  One row per variant of gemm_rw_kernel:
#   (name, K, N, flags, opts, compute dtype, output dtype, (KC, NT, BMR, NS, NW, OCC), ng)
# flags: kinet_gemm_set_flags bits on top of 8 (the resident-weight kernel from M >= 256), which every
#   case sets;  opts, space separated: R residual, Rld residual with ldr = N + 8, LN LayerNorm, A2 the
#   load-time add, s per-column scale, b bias, relu, mask the row mask, ld output rows of N + 8 elements;
# the last two columns are the instantiation and the number of column groups EXPECTED FROM READING
# the launch rules (rw_plan and kRwVariants of csrc/gemm_rw_plan.h; the ring depth worked out by hand
# from the LDS budget): literals, never taken from the library (test_gemm_rw_plan_cpu.py compares the
# planner with them).  M is 17 * BMR - 5 for every case: 17 row tiles, the
# last one ragged (11 of 16 or 27 of 32 rows).
RW_F16ROW, RW_W4, RW_LN6, RW_NOTR, RW_NOSTEM = 131072, 268435456, 4194304, 1073741824, 32
_B, _H, _F = torch.bfloat16, torch.float16, torch.float32
RW_CASES = [
    # K = 64: 128-byte rows, 32-row tiles whatever the epilogue (flag 131072 does not apply)
    ('k64 plain', 64, 256, 0, '', _B, _B, (2, 4, 32, 4, 4, 2), 1),
    ('k64 plain N=264', 64, 264, 0, 's b mask', _H, _F, (2, 4, 32, 4, 4, 2), 2),
    ('k64 R', 64, 200, 0, 'R s b relu mask', _H, _H, (2, 4, 32, 3, 4, 2), 1),
    ('k64 R+LN', 64, 256, 0, 'R LN mask', _B, _B, (2, 4, 32, 3, 4, 2), 1),
    ('k64 LN', 64, 200, 0, 'LN', _H, _H, (2, 4, 32, 4, 4, 2), 1),
    ('k64 A2', 64, 256, 0, 'A2 b', _B, _H, (2, 4, 32, 4, 4, 2), 1),
    ('k64 A2 ld', 64, 264, 0, 'A2 ld mask', _B, _F, (2, 4, 32, 4, 4, 2), 2),
    # K = 128
    ('k128 plain', 128, 256, 0, '', _B, _B, (4, 4, 32, 4, 4, 2), 1),
    ('k128 plain 16-row', 128, 264, RW_F16ROW, 's b mask', _H, _H, (4, 4, 16, 4, 4, 2), 2),
    ('k128 R', 128, 200, 0, 'R s b relu mask', _B, _B, (4, 4, 16, 4, 4, 2), 1),
    ('k128 R 8-wave', 128, 456, 0, 'R b', _H, _H, (4, 4, 16, 4, 8, 1), 1),
    ('k128 R N>256 4-wave', 128, 520, RW_W4, 'Rld b mask', _B, _H, (4, 4, 16, 4, 4, 2), 3),
    ('k128 R+LN', 128, 256, 0, 'R LN', _H, _H, (4, 4, 16, 4, 4, 2), 1),
    ('k128 LN', 128, 200, 0, 'LN mask', _B, _F, (4, 4, 16, 4, 4, 2), 1),
    ('k128 A2', 128, 264, 0, 'A2 b', _B, _F, (4, 4, 16, 4, 4, 2), 2),
    ('k128 N=1024', 128, 1024, 0, 'b', _B, _H, (4, 4, 32, 4, 4, 2), 4),
    # K = 256
    ('k256 plain', 256, 200, 0, 's b relu', _H, _H, (8, 4, 32, 4, 4, 2), 1),
    ('k256 plain ld', 256, 264, 0, 'b ld mask', _B, _B, (8, 4, 32, 4, 4, 2), 2),
    ('k256 plain 16-row', 256, 256, RW_F16ROW, '', _B, _F, (8, 4, 16, 4, 4, 2), 1),
    ('k256 R', 256, 256, 0, 'Rld b', _B, _H, (8, 4, 16, 4, 4, 2), 1),
    ('k256 R 8-wave', 256, 512, 0, 'R s b relu mask', _B, _B, (8, 4, 16, 4, 8, 1), 1),
    ('k256 R 8-wave N=520', 256, 520, 0, 'R b ld', _H, _H, (8, 4, 16, 4, 8, 1), 2),
    ('k256 R N>256 4-wave', 256, 456, RW_W4, 'R s b mask', _H, _H, (8, 4, 16, 4, 4, 2), 2),
    ('k256 R+LN', 256, 200, 0, 'R LN mask', _B, _B, (8, 4, 16, 4, 4, 2), 1),
    ('k256 R+LN N=256', 256, 256, 0, 'R LN', _H, _H, (8, 4, 16, 4, 4, 2), 1),
    ('k256 LN', 256, 256, 0, 'LN', _H, _F, (8, 4, 16, 4, 4, 2), 1),
    ('k256 A2', 256, 200, 0, 'A2 b mask', _H, _H, (8, 4, 16, 4, 4, 2), 1),
    ('k256 A2 N=264', 256, 264, 0, 'A2', _B, _F, (8, 4, 16, 4, 4, 2), 2),
    ('k256 N=1024', 256, 1024, 0, 's b', _H, _F, (8, 4, 32, 4, 4, 2), 4),
    # K = 512: 128-column groups of 4 waves (NT = 2), 256-column groups of 8
    ('k512 N=128', 512, 128, 0, '', _B, _B, (16, 2, 16, 4, 4, 2), 1),
    ('k512 N=72', 512, 72, 0, 's b relu mask', _H, _F, (16, 2, 16, 4, 4, 2), 1),
    ('k512 8-wave', 512, 256, 0, 's b mask', _H, _H, (16, 2, 16, 4, 8, 1), 1),
    ('k512 8-wave N=200', 512, 200, 0, 'b ld', _B, _H, (16, 2, 16, 4, 8, 1), 1),
    ('k512 N=136 4-wave', 512, 136, RW_W4, 's b', _B, _B, (16, 2, 16, 4, 4, 2), 2),
    ('k512 N=256 4-wave', 512, 256, RW_W4, 'b mask', _B, _F, (16, 2, 16, 4, 4, 2), 2),
    # K = 288: 36-chunk rows (their own swizzle), 16-row tiles, 12 columns per lane (NT = 3) but for
    # the 9-wave LayerNorm group (NT = 2)
    ('k288 A2 8-wave', 288, 384, 0, 'A2 b', _B, _H, (9, 3, 16, 4, 8, 1), 1),
    ('k288 A2 8-wave N=328', 288, 328, 0, 'A2 mask', _H, _F, (9, 3, 16, 4, 8, 1), 1),
    ('k288 A2 N=192', 288, 192, 0, 'A2 b', _H, _H, (9, 3, 16, 3, 4, 2), 1),
    ('k288 A2 N=384 4-wave', 288, 384, RW_W4, 'A2 b ld', _B, _B, (9, 3, 16, 3, 4, 2), 2),
    ('k288 R+LN 9-wave', 288, 288, 0, 'R LN mask', _B, _B, (9, 2, 16, 4, 9, 1), 1),
    ('k288 R+LN 9-wave N=280', 288, 280, 0, 'R LN', _H, _H, (9, 2, 16, 4, 9, 1), 1),
    ('k288 R+LN 6-wave', 288, 288, RW_LN6, 'R LN', _H, _H, (9, 3, 16, 4, 6, 1), 1),
    ('k288 R+LN 6-wave N=280', 288, 280, RW_LN6, 'R LN mask', _B, _B, (9, 3, 16, 4, 6, 1), 1),
    ('k288 LN 9-wave', 288, 288, 0, 'LN', _H, _F, (9, 2, 16, 4, 9, 1), 1),
    ('k288 LN 9-wave N=280', 288, 280, 0, 'LN mask', _B, _B, (9, 2, 16, 4, 9, 1), 1),
    ('k288 LN 6-wave', 288, 288, RW_LN6, 'LN mask', _B, _F, (9, 3, 16, 4, 6, 1), 1),
    ('k288 LN 6-wave N=280', 288, 280, RW_LN6, 'LN', _H, _H, (9, 3, 16, 4, 6, 1), 1),
    ('k288 R', 288, 200, 0, 'R s b relu mask', _B, _H, (9, 3, 16, 3, 4, 2), 2),
    ('k288 R N=136', 288, 136, 0, 'Rld b', _H, _H, (9, 3, 16, 3, 4, 2), 1),
    ('k288 N=1728 8-wave', 288, 1728, 0, 'b', _B, _B, (9, 3, 16, 4, 8, 1), 5),
    ('k288 N=1728 4-wave', 288, 1728, RW_W4, 'b mask', _H, _F, (9, 3, 16, 4, 4, 2), 9),
    ('k288 N=288', 288, 288, 0, 's b ld', _B, _B, (9, 3, 16, 4, 4, 2), 2),
    ('k288 N=392', 288, 392, 0, 'b mask', _H, _H, (9, 3, 16, 4, 8, 1), 2),
]
RW_TILES = 17
RW_CONFIG_FIELDS = ('KC', 'NT', 'BMR', 'NS', 'NW', 'OCC', 'HAS_R', 'LN', 'HAS_A2', 'CR', 'PREP', 'out_bytes', 'P',
                    'ng', 'n_mtiles')
# grid cap -> workgroups per column group for 17 row tiles: one tile each; one workgroup walking all
# 17 (every ring slot reused 4-8 times); 6 / 6 / 5 tiles with the ragged tile last; one workgroup with 2
# tiles and 15 with 1 (the prefetch guard cnt < NS - 1 on both sides)
RW_CAPS = {0: 17, 1: 1, 3: 3, 16: 16}


def rw_rows(bmr):
    return RW_TILES * bmr - 5


def rw_opts(case):
    return set(case[4].replace('Rld', 'R Rld').split())


def rw_expected(cfg, ng, has_r, ln, a2, out_dtype, cap, cr=0, prep=0, tiles=RW_TILES):
    """The record kinet_gemm_rw_last_config must return for a table row under grid cap `cap`."""
    p = tiles if cap == 0 else min(cap, tiles)
    vals = tuple(cfg) + (int(has_r), int(ln), int(a2), cr, prep, 4 if out_dtype == torch.float32 else 2, p, ng, tiles)
    return dict(zip(RW_CONFIG_FIELDS, vals))


def rw_mask(M, bmr):
    """Masked rows: the first row, the first and the last row of a tile, a whole tile, the last
    (ragged) row."""
    m = torch.zeros(M, dtype=torch.bool)
    m[0] = m[2 * bmr] = m[4 * bmr - 1] = m[M - 1] = True
    m[6 * bmr:7 * bmr] = True
    return m


def _rw_seed(name, cls):
    return sum(map(ord, name)) * 131 + (0 if cls == 'exact' else 5)


def rw_inputs(case, cls, offset=0.0):
    """Every operand of one table row as CPU tensors (f32 holding values of the operand types), and
    its f64 reference.  cls 'exact' / 'generic' as for the tiled kernel; LayerNorm rows take exact
    matrix operands whatever cls says, an f32 bias of offset + randn, a residual of randn rounded to the
    output type (test_ln_epilogue_direct_gpu.py's rule) and return ln = (gamma, beta).
    A2: exact class -- x2 multiples of 1/2 in [-1, 1], so x + x2 is exact in bf16 and f16 (multiples
    of 1/2 up to 2, products multiples of 1/16 up to 1/2: sums still exact in f32); generic class --
    the reference's operand is (x + x2) rounded once to the operand type, as the kernel's is.
    Returns a dict: x, w, x2, scale, bias, res, relu, mask, ln, acc, absprod, pre, maj (pre: the f64
    epilogue value before LayerNorm and before the row mask)."""
    name, K, N, _, _, cdt, odt, cfg, _ = case
    o = rw_opts(case)
    M = rw_rows(cfg[2])
    ln = 'LN' in o
    if ln:
        cls = 'exact'
    g = torch.Generator().manual_seed(_rw_seed(name, cls) + int(offset))
    x, w, acc, ap = gemm_case(M, N, K, cdt, cls)
    d = dict(x=x, w=w, x2=None, scale=None, bias=None, res=None, relu='relu' in o, mask=None, ln=None)
    if 'A2' in o:
        x2 = exact_x((M, K), g) if cls == 'exact' else torch.randn(M, K, generator=g).to(cdt).float()
        a = (x + x2).to(cdt).double()
        acc, ap = a @ w.double().T, a.abs() @ w.double().abs().T
        d['x2'] = x2
    if ln:
        d['bias'] = offset + torch.randn(N, generator=g)
        if 'R' in o:
            d['res'] = torch.randn(M, N, generator=g).to(odt).float()
        d['ln'] = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g))
    else:
        if 's' in o or 'b' in o:
            scale, bias = exact_epilogue(N, g) if cls == 'exact' else generic_epilogue(N, g)
            d['bias'] = bias
            if 's' in o:
                d['scale'] = scale
        if 'R' in o:
            d['res'] = exact_res((M, N), g) if cls == 'exact' else torch.randn(M, N, generator=g).to(odt).float()
    if 'mask' in o:
        d['mask'] = rw_mask(M, cfg[2])
    d['acc'], d['absprod'] = acc, ap
    d['pre'], d['maj'] = epilogue64(acc, d['scale'], d['bias'], d['res'], d['relu'])
    return d


def rw_masked(v, mask):
    return v if mask is None else torch.where(mask.reshape(-1, 1), torch.zeros_like(v), v)


def rw_ln_check(got, inp, odt, eps=1e-5):
    """(worst err / bound, number of elements over it) of a LayerNorm row's output `got` under
    test_ln_epilogue_direct_gpu.py's bound: one rounding of a 16-bit output of the f64 result + 4x
    the maximum error of torch's CPU f32 layer_norm of the same pre-activation; masked rows are 0."""
    gam, bet = inp['ln']
    ref, t = ln_epilogue_yardstick(inp['pre'], gam, bet, eps)
    ref = rw_masked(ref, inp['mask'])
    err = (got.double() - ref).abs()
    tol = OUT_ROUND[odt] * ref.abs() + 4 * t
    return float((err / tol).max()), int((err > tol).sum())


def rw_generic_ratio(got, inp, K, odt):
    """Worst err / gemm_generic_bound of the (M, N) output `got` of a case without LayerNorm."""
    ref = rw_masked(inp['pre'], inp['mask'])
    bound = gemm_generic_bound(inp['absprod'], K, inp['maj'], ref, odt, inp['scale'])
    return float(((got.double() - ref).abs() / bound).max())


# Head-major stores: (name, K, head_dim or 'split', flags, compute dtype, output dtype, config, ng);
# N = K (the value projections), B = 7 x S = 77 rows on 32-row tiles, B = 3 x S = 89 on 16-row tiles.
RW_HM_CASES = [
    ('hm32 k256 transpose', 256, 32, 0, _B, _H, (8, 4, 32, 4, 4, 2), 1),
    ('hm32 k256 direct', 256, 32, RW_NOTR, _B, _H, (8, 4, 32, 4, 4, 2), 1),
    ('hm32 k256 transpose 16-row', 256, 32, RW_F16ROW, _H, _H, (8, 4, 16, 4, 4, 2), 1),
    ('hm32 k256 direct 16-row', 256, 32, RW_F16ROW | RW_NOTR, _B, _B, (8, 4, 16, 4, 4, 2), 1),
    ('hm36 k288', 288, 36, 0, _B, _H, (9, 3, 16, 4, 4, 2), 2),
    ('hm48 k288', 288, 48, 0, _H, _H, (9, 3, 16, 4, 4, 2), 2),
    ('hm split k288', 288, 'split', 0, _B, _H, (9, 3, 16, 4, 4, 2), 2),
    ('hm split k288 bf16', 288, 'split', 0, _B, _B, (9, 3, 16, 4, 4, 2), 2),
]


def rw_hm_batch(bmr):
    return (7, 77) if bmr == 32 else (3, 89)


def rw_hm_layout(rows, B, S, h):
    """(M, d) rows in the head-major layout the kernel stores: (d // h, B, S, h)."""
    M, d = rows.shape
    return rows.view(B, S, d // h, h).permute(2, 0, 1, 3).contiguous()


def rw_hm_rows(y):
    """A head-major output (heads, B, S, h) back in (row, column) order, as the tests compare it."""
    heads, B, S, h = y.shape
    return y.permute(1, 2, 0, 3).reshape(B * S, heads * h)


# Conv-row mode (family 5): (name, (KH, Cin, Cout, stride (h, w), pad_h, Hin, Win), flags, opts, config,
# ng).  Two images of Hout = 4 rows of Wout = 33 pixels: M = 264 rows, 9 tiles of 32 or 17 of 16, so tiles
# straddle output rows (33 is odd) and the image boundary (row 132 sits inside a tile of either height).
#   strided 1x1: Cin = 256, stride 2, input 7 x 65;
#   the tap-folded stem form, 7 x 1 taps of 24 channels (K = 168 of the kernel's 256: the chunks past K
#     read zeros), vertical stride 2 / pad 3 (flag 32 keeps the dedicated stem kernel off it);
#   3 x 1 taps of 64 channels with pad 3 over 3 input rows: output rows 0 and 3 read padding only.
RW_CONV_CASES = [
    ('ds 256->256', (1, 256, 256, (2, 2), 0, 7, 65), 0, '', (8, 4, 32, 4, 4, 2), 1),
    ('ds 256->512', (1, 256, 512, (2, 2), 0, 7, 65), 0, 's b relu', (8, 4, 32, 4, 4, 2), 2),
    ('ds 256->256 16-row', (1, 256, 256, (2, 2), 0, 7, 65), RW_F16ROW, 's b', (8, 4, 16, 4, 4, 2), 1),
    ('ds 256->512 16-row', (1, 256, 512, (2, 2), 0, 7, 65), RW_F16ROW, '', (8, 4, 16, 4, 4, 2), 2),
    ('stem 7x1 N=64', (7, 24, 64, (2, 1), 3, 8, 33), RW_NOSTEM, 's b relu', (8, 2, 32, 4, 4, 2), 1),
    ('stem 7x1 N=128 16-row', (7, 24, 128, (2, 1), 3, 8, 33), RW_NOSTEM | RW_F16ROW, '', (8, 2, 16, 4, 4, 2), 1),
    ('taps 3x1 N=128', (3, 64, 128, (2, 1), 3, 3, 33), RW_NOSTEM, 's b', (8, 2, 32, 4, 4, 2), 1),
    ('taps 3x1 N=64 16-row', (3, 64, 64, (2, 1), 3, 3, 33), RW_NOSTEM | RW_F16ROW, 'b relu', (8, 2, 16, 4, 4, 2), 1),
]
RW_CONV_BATCH, RW_CONV_ROWS = 2, 264

# Sampling records (PREP), 3 frames x 89 queries x 8 heads: (name, flags, x_add, config, ng): one 8-wave
# 384-column group; two 4-wave groups with the load-time add (2 ring slots, 3 workgroups per CU) and
# without it
PREP_CASES = [('records 8-wave', 0, True, (8, 3, 16, 4, 8, 1), 1),
              ('records 4-wave A2', RW_W4, True, (8, 3, 16, 2, 4, 3), 2),
              ('records 4-wave', 0, False, (8, 3, 16, 4, 4, 2), 2)]


@functools.lru_cache(maxsize=None)
def rw_conv_inputs(name, dtype, cls):
    """(x NHWC, w (Cout, KH, 1, Cin), scale, bias, acc64, |x| * |w|) of a conv-row case."""
    geo, opts = next((c[1], c[3]) for c in RW_CONV_CASES if c[0] == name)
    KH, Cin, Cout, stride, pad_h, Hin, Win = geo
    K = KH * Cin
    g = torch.Generator().manual_seed(_rw_seed(name, cls))
    if cls == 'exact':
        x, w = exact_x((RW_CONV_BATCH, Hin, Win, Cin), g), exact_w((Cout, KH, 1, Cin), K, g)
        scale, bias = exact_epilogue(Cout, g)
    else:
        x, w = generic_operands((RW_CONV_BATCH, Hin, Win, Cin), (Cout, KH, 1, Cin), K, dtype, g)
        scale, bias = generic_epilogue(Cout, g)
    o = opts.split()
    return (x, w, scale if 's' in o else None, bias if 'b' in o else None, conv64(x, w, stride, (pad_h, 0)),
            conv64(x.abs(), w.abs(), stride, (pad_h, 0)))


# ============================ MSDA forward sampling (csrc/msda.hip, csrc/msda_enc.hip)
def msda_sample_ref(value, shapes, loc, attw):
    """ms_deform_im2col's forward (ms_deform_im2col_cuda.cuh:165-237) in plain torch f64: value
    (B, S, M, D), shapes [(H, W)] * L, loc (B, Lq, M, L, P, 2) normalised (x, y), attw (B, Lq, M, L, P).
    Per tap h = y H - 0.5, w = x W - 0.5; outside (-1, H) x (-1, W) it adds 0; else the four corners
    (floor(h) + {0, 1}, floor(w) + {0, 1}) inside the level, weighted (1 - lh | lh) (1 - lw | lw) a.
    That is bilinear interpolation of the level padded with zeros, continuous in (h, w) everywhere.
    Returns, each (B, Lq, M * D) unless said:
      out    the output
      A      sum |a w_corner v|, the running-error majorant;  A_lvl (L, ...) its split per level
      V      sum |v| over the in-level corners of taps with a != 0 (what an ABSOLUTE tap-weight error multiplies)
      G_lvl  (L, ...) per level: sum over its taps of a (gx + gy), gx (gy) the largest |difference| of
             horizontally (vertically) adjacent pixels of the zero-padded level within rows
             floor(h) - 1 .. floor(h) + 2, columns floor(w) - 1 .. floor(w) + 2: every cell a location
             error below one pixel can reach.  Moving every tap of level l by at most d_l pixels per
             axis moves the output by at most sum_l G_lvl[l] d_l;  G = sum_l G_lvl[l]."""
    value, loc, attw = value.double(), loc.double(), attw.double()
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    bi = torch.arange(B).view(B, 1, 1, 1)
    mi = torch.arange(M).view(1, 1, M, 1)
    out = torch.zeros(B, Lq, M, D, dtype=torch.float64)
    A_lvl = torch.zeros(L, B, Lq, M, D, dtype=torch.float64)
    G_lvl, V = torch.zeros_like(A_lvl), torch.zeros_like(out)
    start = 0
    for l, (H, W) in enumerate((int(h), int(w)) for h, w in shapes):
        v = value[:, start:start + H * W]                                   # (B, H W, M, D)
        h = loc[:, :, :, l, :, 1] * H - 0.5                                 # (B, Lq, M, P)
        w = loc[:, :, :, l, :, 0] * W - 0.5
        a = attw[:, :, :, l, :]
        valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h), torch.floor(w)
        lh, lw = h - hl, w - wl
        for dy, wy in ((0, 1 - lh), (1, lh)):
            for dx, wx in ((0, 1 - lw), (1, lw)):
                r, c = hl + dy, wl + dx
                ok = valid & (r >= 0) & (r < H) & (c >= 0) & (c < W)
                idx = (r.clamp(0, H - 1) * W + c.clamp(0, W - 1)).long()
                vc = v[bi, idx, mi] * ok[..., None]                         # (B, Lq, M, P, D)
                t = (a * wy * wx)[..., None] * vc
                out += t.sum(3)
                A_lvl[l] += t.abs().sum(3)
                V += (vc.abs() * (a != 0)[..., None]).sum(3)
        # the slope: |differences| of the level padded by 3 zero pixels, max-pooled over the 4 x 4 footprint
        img = F.pad(v.permute(0, 2, 3, 1).reshape(B, M * D, H, W), (3, 3, 3, 3))
        gx = F.max_pool2d((img[..., :, 1:] - img[..., :, :-1]).abs(), (4, 3), 1)     # (B, M D, H + 3, W + 3)
        gy = F.max_pool2d((img[..., 1:, :] - img[..., :-1, :]).abs(), (3, 4), 1)
        g = (gx + gy).reshape(B, M, D, (H + 3) * (W + 3)).permute(0, 3, 1, 2)      # (B, pix, M, D)
        gidx = ((hl + 2).clamp(0, H + 2) * (W + 3) + (wl + 2).clamp(0, W + 2)).long()
        G_lvl[l] = (a[..., None] * g[bi, gidx, mi]).sum(3)
        start += H * W
    f = lambda t: t.reshape(*t.shape[:-2], M * D)
    return {'out': f(out), 'A': f(A_lvl.sum(0)), 'A_lvl': f(A_lvl), 'V': f(V), 'G_lvl': f(G_lvl), 'G': f(G_lvl.sum(0))}


# ---- the strip plan of the encoder kernel (msda_enc.hip: plan_layout, enc_plan, enc_tiles) ----
ENC_MAIN, ENC_TAIL, ENC_HALO, ENC_QT = 2544, 2256, 4, 16

# (name, level shapes, batch, heads, channels, forced strips) -> (fl, nstrip, used), Lq = S.  Written down
# by reading plan_layout / enc_plan for 256 compute units:
#   region of a staged level: cap = min(H + 2, ceil(H / n) + 3 + 2 * 4) rows, ceil16(cap W + 2) map pixels,
#   after a zero margin of ceil16(widest staged W + 2); budget 2544 pixels (36 channels: 2256);
#   fl = the fewest gathered levels that fit at some n <= min(64, tiles // 16); the automatic n is the first
#   >= the smallest fitting one that fills 90 % of a round of 256 workgroups (8 maps: never below 29, so the
#   smallest fitting n); a forced n is honoured in [smallest fitting, min(64, tiles // 16)].
#   'all' n = 1: 48 + ceil16(27*40+2) + ceil16(17*20+2) + ceil16(10*10+2) + ceil16(6*5+2) = 48+1088+352+112+32
#   'wide1': level 0 needs >= 12 rows of 200 + margin 208 > 2544 with the others; levels 1-3: 112+704+256+112
#   'wide2': level 1 (190 wide, 14 rows) does not fit beside 2-3; levels 2-3: 32 + ceil16(8*30+2) + ceil16(5*15+2)
#   'wide2s': level 2 = 13 x 180: cap 12 (n >= 13: ceil(13/13) + 11) -> 192 + 2176 + 144; with 36 channels
#             12 * 180 + 192 > 2256 at every n, level 3 alone: 32 + ceil16(7*20+2)
#   'wide3': level 2 (7 rows of 220) + level 3 (5 rows of 216) exceed the map; level 3: 224 + ceil16(5*216+2)
#   'tall1': level 0 (200 wide) never fits; levels 1-3 are taller than cap from n = 2 (n = 4: 21, 19, 16 rows)
MSDA_ENC_GEO = {
    'all': ((25, 40), (15, 20), (8, 10), (4, 5)),
    'wide1': ((10, 200), (5, 100), (3, 50), (2, 25)),
    'wide2': ((10, 200), (12, 190), (6, 30), (3, 15)),
    'wide2s': ((10, 200), (12, 190), (13, 180), (5, 20)),
    'wide3': ((4, 230), (3, 225), (5, 220), (3, 216)),
    'tall1': ((12, 200), (40, 30), (30, 20), (20, 10)),
}
MSDA_ENC_REFUSED = ((20, 250), (20, 250), (20, 250), (20, 250))
MSDA_ENC_CASES = [
    ('all', 1, 8, 32, 0, (0, 1, 1632)), ('all', 1, 8, 32, 1, (0, 1, 1632)), ('all', 1, 8, 32, 2, (0, 2, 1520)),
    ('all', 1, 8, 32, 3, (0, 3, 1344)), ('all', 3, 8, 32, 3, (0, 3, 1344)), ('all', 1, 5, 32, 3, (0, 3, 1344)), ('all', 2, 5, 32, 3, (0, 3, 1344)),
    ('all', 1, 8, 36, 3, (0, 3, 1344)), ('all', 1, 8, 32, 13, (0, 1, 1632)),          # 13 > tiles // 16 = 5: ignored
    ('wide1', 1, 8, 32, 0, (1, 1, 1184)), ('wide1', 1, 8, 32, 3, (1, 3, 1184)), ('wide1', 1, 8, 36, 0, (1, 1, 1184)),
    ('wide2', 1, 8, 32, 0, (2, 1, 368)), ('wide2', 1, 8, 32, 4, (2, 4, 368)),
    ('wide2s', 1, 8, 32, 0, (2, 13, 2512)), ('wide2s', 1, 8, 32, 3, (2, 13, 2512)),  # 3 < 13: ignored
    ('wide2s', 1, 8, 36, 0, (3, 1, 176)), ('wide2s', 1, 8, 36, 3, (3, 3, 176)),
    ('wide3', 1, 8, 32, 0, (3, 1, 1312)), ('wide3', 1, 8, 32, 2, (3, 2, 1312)),
    ('tall1', 1, 8, 32, 0, (1, 1, 2176)), ('tall1', 1, 8, 32, 4, (1, 4, 1232)), ('tall1', 1, 8, 36, 4, (1, 4, 1232)),
    ('tall1', 1, 8, 32, 13, (1, 13, 928)),
]


def msda_enc_expected(name, batch, heads, channels, forced):
    return next(c[5] for c in MSDA_ENC_CASES if c[:5] == (name, batch, heads, channels, forced))


def msda_enc_caps(shapes, fl, n):
    """Rows per staged region (0 for a gathered level), plan_layout's rule."""
    return [0 if l < fl else min(H + 2, (H + n - 1) // n + 3 + 2 * ENC_HALO) for l, (H, W) in enumerate(shapes)]


def msda_enc_windows(shapes, fl, n, order=None):
    """enc_tiles' staged rows restated in f64: per strip s and staged level l the window [r, r + cap - 1]
    (a footprint is read from LDS iff r <= floor(h) < r + cap - 1) -> (tile -> strip (ntile,), r (n, L)).
    The strip's query rows come from its level-0 tiles (or every tile's first query when it has none);
    hmin = floor(ylo H - 0.5), hmax = floor(yhi H - 0.5) + 1, r = hmin - max(0, (cap - (hmax - hmin + 1)) // 2)
    clamped to [-1, H + 1 - cap].  The kernel computes ylo H - 0.5 in f32: where that lands within
    rounding of an integer its window may sit one row off this one, so callers keep one row of slack."""
    hw = [h * w for h, w in shapes]
    starts = np.concatenate([[0], np.cumsum(hw)]).astype(np.int64)
    Lq = int(starts[-1])
    ntile = (Lq + ENC_QT - 1) // ENC_QT
    order = np.arange(ntile) if order is None else np.asarray(order)
    caps = msda_enc_caps(shapes, fl, n)
    strip_of = np.zeros(ntile, dtype=np.int64)
    win = np.zeros((n, len(shapes)), dtype=np.int64)
    for s in range(n):
        t0, t1 = s * ntile // n, (s + 1) * ntile // n
        q0 = order[t0:t1] * ENC_QT
        strip_of[order[t0:t1]] = s
        H0, W0 = shapes[0]
        in0 = q0 < starts[1]
        if in0.any():
            qb = np.minimum(q0[in0] + ENC_QT, starts[1]) - 1
            ylo, yhi = ((q0[in0] // W0).min() + 0.5) / H0, ((qb // W0).max() + 0.5) / H0
        else:
            lv = np.searchsorted(starts, q0, side='right') - 1
            y = ((q0 - starts[lv]) // np.array([w for _, w in shapes])[lv] + 0.5) / np.array([h for h, _ in shapes])[lv]
            ylo, yhi = y.min(), y.max()
        for l in range(fl, len(shapes)):
            H, cap = shapes[l][0], caps[l]
            hmin, hmax = math.floor(ylo * H - 0.5), math.floor(yhi * H - 0.5) + 1
            r = hmin - max(0, cap - (hmax - hmin + 1)) // 2
            win[s, l] = max(-1, min(r, H + 1 - cap))
    return strip_of, win


# ---- problems: two operand classes ----
def msda_hm(offlog, M, L=4, P=4):
    """(B, Lq, M L P 3) [offsets | logits] -> (M, B, Lq, L P 3) per-head [offsets | logits], f16."""
    B, Lq, _ = offlog.shape
    off = offlog[..., :M * L * P * 2].reshape(B, Lq, M, L * P * 2)
    lg = offlog[..., M * L * P * 2:].reshape(B, Lq, M, L * P)
    return torch.cat([off, lg], -1).permute(2, 0, 1, 3).contiguous().half()


def msda_pixel_refs(shapes, B):
    """The encoder's reference points with valid ratios 1: query q = pixel (i, j) of its level ->
    ((j + .5) / W, (i + .5) / H) at every level; also each query's (level, row, col)."""
    pts, meta = [], []
    for l, (h, w) in enumerate(shapes):
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
        pts.append(torch.stack([(xx.reshape(-1) + 0.5) / w, (yy.reshape(-1) + 0.5) / h], -1))
        meta.append(torch.stack([torch.full((h * w,), l), yy.reshape(-1).long(), xx.reshape(-1).long()], -1))
    r = torch.cat(pts, 0)
    return r[None, :, None, :].expand(B, -1, len(shapes), -1).contiguous(), torch.cat(meta, 0)


MSDA_COLD = -30000.0     # a cold logit: exp(-30000) is exactly 0 in f32 and -30000 rounds to a finite f16
ADDR_CATS = ('near', 'far', 'row-1', 'rowH-1', 'col-1', 'colW-1', 'win_first', 'win_last')


@functools.lru_cache(maxsize=None)
def msda_addr_case(shapes, B, M, Lq, ref_dim, D=32, P=4, plan=None, order=None, seed=0):
    """The addressing class.  Values 4 * integers in [-8, 8] (exact in bf16 / f16, and a quarter of a sum
    of four is still an integer).  Per (b, q, head m) ONE tap has logit 0 and the others MSDA_COLD: the
    softmax is exactly (1, 0, ..., 0).  The hot tap (l, p) = ((q + m) % L, (q // L + m) % P) rotates over
    the L * P taps with the query index.  Per (b, q, level l) one TARGET: a pixel centre (h, w) = (row, col)
    -- one pixel read -- or, every other query, the cell corner (row + .5, col + .5) -- four pixels at
    weight 1/4.  The offsets are small multiples of 1/2 (exact in f16), shared by the level's taps, and the
    reference point is target - offset term, rounded to f32: the f64 location of the hot tap is within one
    f32 rounding of the target.
    Target categories rotate with (q // 16 + l): 'near' (within 2 rows of the query's own row), 'far' (more
    than cap rows from it, where the level is taller than its staged window), row -1, row H - 1, column -1,
    column W - 1, and the first / last rows of the strip's staged window (plan = (fl, nstrip), tile order
    `order`; without a plan the categories fold onto the first six and 'far' means any other row).
    -> dict(value (B, S, M, D) f64, offlog (B, Lq, 3 M L P) f32, refs (B, Lq, L, ref_dim) f32, cat (B, Lq, L) index
    into ADDR_CATS, hot (B, Lq, M) hot level, refs64 the reference points before their rounding to f32: the
    records front end takes none, its records are built from these)."""
    g = torch.Generator().manual_seed(seed + 7 * Lq + M)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    value = 4.0 * torch.randint(-8, 9, (B, S, M, D), generator=g).double()
    q = torch.arange(Lq)
    if Lq == S:
        _, meta = msda_pixel_refs(shapes, 1)
        qy = (meta[:, 1].double() + 0.5) / torch.tensor([shapes[l][0] for l in meta[:, 0].tolist()], dtype=torch.float64)
        qx = (meta[:, 2].double() + 0.5) / torch.tensor([shapes[l][1] for l in meta[:, 0].tolist()], dtype=torch.float64)
    else:
        qy, qx = torch.rand(Lq, generator=g).double(), torch.rand(Lq, generator=g).double()
    fl, n = plan if plan is not None else (L, 1)
    caps = msda_enc_caps(shapes, fl, n)
    strip_of, win = msda_enc_windows(shapes, fl, n, order) if plan is not None and Lq == S else (None, None)
    offlog = torch.zeros(B, Lq, 3 * M * L * P)
    refs = torch.zeros(B, Lq, L, ref_dim, dtype=torch.float64)
    cat = torch.zeros(B, Lq, L, dtype=torch.long)
    off = torch.randint(-6, 7, (B, Lq, L, 2), generator=g).double() / 2          # (x, y) raw offsets
    if ref_dim == 4:
        refs[..., 2:] = torch.randint(1, 5, (B, Lq, L, 2), generator=g).double() / 8      # w, h in {1/8 .. 1/2}
    for l, (H, W) in enumerate(shapes):
        own_r = torch.floor(qy * H).long().clamp(0, H - 1)[None].expand(B, -1)
        own_c = torch.floor(qx * W).long().clamp(0, W - 1)[None].expand(B, -1)
        k = ((q // 16 + l)[None] + torch.arange(B)[:, None]) % len(ADDR_CATS)
        dr = torch.randint(-2, 3, (B, Lq), generator=g)
        dc = torch.randint(-2, 3, (B, Lq), generator=g)
        row, col = (own_r + dr).clamp(0, H - 1), (own_c + dc).clamp(0, W - 1)
        c_near = torch.zeros_like(k)
        staged = l >= fl and strip_of is not None
        far_ok = H > caps[l] if plan is not None and l >= fl else H > 6
        gap = caps[l] + 1 if plan is not None and l >= fl else 3
        up, dn = own_r - gap - dr.abs(), own_r + gap + dr.abs()
        far_row = torch.where(up >= 0, up, dn)
        is_far = (k == 1) & far_ok & (far_row >= 0) & (far_row < H)
        row = torch.where(is_far, far_row, row)
        is_top, is_bot = k == 2, k == 3
        row = torch.where(is_top, torch.full_like(row, -1), torch.where(is_bot, torch.full_like(row, H - 1), row))
        is_left, is_right = k == 4, k == 5
        col = torch.where(is_left, torch.full_like(col, -1), torch.where(is_right, torch.full_like(col, W - 1), col))
        kk = torch.where(is_far, 1, torch.where(is_top, 2, torch.where(is_bot, 3, torch.where(is_left, 4, torch.where(
            is_right, 5, c_near)))))
        if staged:
            # rows r, r + 1 and r + cap - 3 .. r + cap - 1 of the query's strip: both sides of either edge of
            # `r <= floor(h) < r + cap - 1` whichever way the kernel's f32 window rounds
            r0 = torch.as_tensor(win[strip_of[(q // 16).numpy()], l])[None].expand(B, -1)
            first = (r0 + (dr % 2)).clamp(-1, H - 1)
            last = (r0 + caps[l] - 3 + (dr % 3)).clamp(-1, H - 1)
            row = torch.where(k == 6, first, torch.where(k == 7, last, row))
            kk = torch.where(k == 6, 6, torch.where(k == 7, 7, kk))
        cat[:, :, l] = kk
        corner = (((q // 2)[None] + torch.arange(B)[:, None]) % 2).double() * 0.5          # cell corner every other pair
        # a corner target on the last row / column would be half outside: fine (zero padding), kept
        th, tw = row.double() + corner, col.double() + corner
        ty, tx = (th + 0.5) / H, (tw + 0.5) / W
        ox, oy = off[:, :, l, 0], off[:, :, l, 1]
        if ref_dim == 2:
            refs[:, :, l, 0], refs[:, :, l, 1] = tx - ox / H, ty - oy / W          # the (H, W) normaliser on (x, y)
        else:
            refs[:, :, l, 0] = tx - ox / P * refs[:, :, l, 2] * 0.5
            refs[:, :, l, 1] = ty - oy / P * refs[:, :, l, 3] * 0.5
    n_tap = M * L * P
    o = off[:, :, None, :, None, :].expand(B, Lq, M, L, P, 2)
    offlog[..., :2 * n_tap] = o.reshape(B, Lq, 2 * n_tap).float()
    m = torch.arange(M)
    hot_l = (q[:, None] + m[None]) % L
    hot_p = (q[:, None] // L + m[None]) % P
    lg = torch.full((B, Lq, M, L * P), MSDA_COLD)
    lg.scatter_(3, (hot_l * P + hot_p)[None, :, :, None].expand(B, -1, -1, -1), 0.0)
    offlog[..., 2 * n_tap:] = lg.reshape(B, Lq, n_tap)
    return {'value': value, 'offlog': offlog, 'refs': refs.float(), 'refs64': refs, 'cat': cat,
            'hot': hot_l[None].expand(B, -1, -1)}


def msda_addr_counts(case, loc, shapes, plan=None, order=None):
    """From the f64 locations: how many hot samples of each staged (or every, without a plan) level fall in
    each category -- recomputed from floor(h), floor(w), not taken from the construction.
    -> {(level, category name): count}."""
    B, Lq, M, L, P, _ = loc.shape
    fl, n = plan if plan is not None else (0, 1)
    caps = msda_enc_caps(shapes, fl, n)
    S = sum(h * w for h, w in shapes)
    strip_of, win = msda_enc_windows(shapes, fl, n, order) if plan is not None and Lq == S else (None, None)
    q = torch.arange(Lq)
    m = torch.arange(M)
    hot_l = (q[:, None] + m[None]) % L
    hot_p = (q[:, None] // L + m[None]) % P
    counts = {}
    _, meta = msda_pixel_refs(shapes, 1) if Lq == S else (None, None)
    for l, (H, W) in enumerate(shapes):
        sel = hot_l == l                                                         # (Lq, M)
        lp = loc[:, :, :, l].gather(3, hot_p[None, :, :, None, None].expand(B, -1, -1, 1, 2))[:, :, :, 0]   # (B, Lq, M, 2)
        hl = torch.floor(lp[..., 1] * H - 0.5 + 1e-3)      # targets sit on multiples of 1/2
        wl = torch.floor(lp[..., 0] * W - 0.5 + 1e-3)
        sel = sel[None].expand(B, -1, -1)
        c = {'row-1': hl == -1, 'rowH-1': hl == H - 1, 'col-1': wl == -1, 'colW-1': wl == W - 1}
        if meta is not None:
            own = torch.floor((meta[:, 1].double() + 0.5) / torch.tensor([shapes[i][0] for i in meta[:, 0].tolist()]) * H)
            dist = (hl - own[None, :, None]).abs()
            c['near'] = dist <= 2
            if plan is not None and l >= fl and H > caps[l]:
                c['far'] = dist > caps[l]
            if strip_of is not None and l >= fl:
                r0 = torch.as_tensor(win[strip_of[(q // 16).numpy()], l]).double()[None, :, None]
                c['win_first'] = (hl >= r0) & (hl <= r0 + 1)
                c['win_last'] = (hl >= r0 + caps[l] - 3) & (hl <= r0 + caps[l] - 1)
                c['surely_staged'] = (hl >= r0 + 1) & (hl < r0 + caps[l] - 2)
                c['surely_far'] = (hl < r0 - 1) | (hl >= r0 + caps[l])
        for name, mask in c.items():
            counts[(l, name)] = int((mask & sel).sum())
    return counts


@functools.lru_cache(maxsize=None)
def msda_generic_case(shapes, B, M, Lq, ref_dim, noise, logits, dtype, D=32, P=4, masked=True, seed=0, f16_offlog=False):
    """The generic class: randn values rounded to `dtype`, offsets noise * randn (raw units: about `noise`
    pixels), logits randn or +-8, references the pixel centres (Lq = S) or uniform, 10 % masked queries."""
    g = torch.Generator().manual_seed(seed + Lq * 13 + M + int(noise * 10) + ref_dim)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, M, D, generator=g).to(dtype)
    n_tap = M * L * P
    off = noise * torch.randn(B, Lq, 2 * n_tap, generator=g)
    lg = torch.randn(B, Lq, n_tap, generator=g) if logits == 'randn' else \
        torch.where(torch.rand(B, Lq, n_tap, generator=g) < 0.5, -8.0, 8.0)
    offlog = torch.cat([off, lg], -1)
    if f16_offlog:
        offlog = offlog.half().float()
    if Lq == S and ref_dim == 2:
        refs = msda_pixel_refs(shapes, B)[0].float()
    else:
        refs = torch.rand(B, Lq, L, ref_dim, generator=g)
        if ref_dim == 4:
            refs[..., 2:] = refs[..., 2:] * 0.5 + 0.05
    qmask = (torch.rand(B, Lq, generator=g) < 0.1) if masked else None
    return {'value': value, 'offlog': offlog, 'refs': refs, 'qmask': qmask}


def msda_chain_ref(case, shapes, M, P=4):
    """raw offsets / logits / references / mask -> msda_prep_ref -> msda_sample_ref, nothing else."""
    L = len(shapes)
    ss = torch.tensor(shapes, dtype=torch.int64)
    prep = msda_prep_ref(case['offlog'], case['refs'], ss, case.get('qmask'), M, L, P)
    samp = msda_sample_ref(case['value'].double(), shapes, prep['loc'], prep['attw'])
    return prep, samp


# ---- bounds ----
LOC_OPS = 7
F16_W = 2.0 ** -11            # one rounding of a tap weight to f16
F16_W_ABS = 2.0 ** -25        # ... of a subnormal one (spacing 2^-24): kinet_amd/build.py passes no flush or
#                               fast-math flag, and the AMDGPU default float mode keeps f16 subnormals


def msda_loc_delta(prep, shapes):
    """(L,) pixels: the most a kernel's f32 tap location (h, w) of level l can differ from the f64 one.
    Counted on the longest variant, per axis: the offset term -- 1 / H (a reciprocal), the product with
    it, or / P * wh * 0.5 -- at most 3 roundings, the sum with the reference point 1, the product with the
    level size 1, the subtraction of 0.5 1: 6, each relative to at most |ref| + |offset term| (locA of
    msda_prep_ref) times the level size, + 0.5;  + 1 for the addressing class, whose reference points are
    themselves rounded to f32 from the exact target: LOC_OPS = 7."""
    d = []
    for l, (H, W) in enumerate(shapes):
        A = prep['locA'][:, :, :, l]
        d.append(LOC_OPS * U32 * max((A[..., 0] * W).max().item(), (A[..., 1] * H).max().item()) + LOC_OPS * U32)
    return torch.tensor(d, dtype=torch.float64)


# c_acc: relative to A, read off each kernel.
#   f32 weights, f32 accumulation (msda_fwd_kernel, msda_fused_kernel): 1 - lh, two products: 3; the fma
#     chain over 16 taps x 4 corners: 64                                           -> 67 * 2^-24
#   msda_fused_fast_kernel: the same, and the weight rounded to f16                -> + 2^-11
#   msda_enc_kernel: the weight to f16 (2^-11); per level 16 packed-f16 multiply-adds, each rounding a
#     partial sum bounded by that level's A: 16 * 2^-11 * A_lvl; the levels' f32 adds, the tail's quad sum: 8
#   records front end: two packed-f16 products make a weight                       -> 2 * 2^-11
#   f16 subnormals (results below 2^-14, spacing 2^-24) round absolutely: F16_W_ABS per tap weight (times the
#     corner's |v|: V), per packed-f16 multiply-add (64 behind an element of the strip kernel) and for an f16 output
C_ACC_F32 = 67 * U32


def msda_addr_bound(samp, shapes, kernel, locA):
    """The addressing class through offsets and references: |d| <= sum_l G_l d_l, plus what keeps the bound
    sound where G is 0 (a flat neighbourhood): the hot corner's weight product, C_ACC_F32 A, and for the
    kernels that round it to f16 F16_W A -- at most 2^-11 * 32 = 1/64.  No accumulation or output term:
    the expected values are integers of at most 6 bits, every partial sum and the output lie within the
    terms above of one, and rounding to nearest cannot move a number away from a representable
    neighbour.  A wrong pixel is off by at least 1 (corner targets) or 4 (centre targets)."""
    d = msda_loc_delta({'locA': locA}, shapes)
    assert d.max().item() < 0.125, 'the geometry is wrong, not the bound'
    c = C_ACC_F32 + (0.0 if kernel == 'f32' else F16_W)
    return (samp['G_lvl'] * d.view(-1, 1, 1, 1)).sum(0) + c * samp['A'] + 1e-30


def msda_bound(samp, shapes, kernel, out_dtype, locA=None, attw_c=None):
    """Per-element bound of |kernel - samp['out']|: c_acc A + out_round |ref| + the subnormal tap weights'
    F16_W_ABS V (f16-weight kernels) + sum_l G_l d_l (locA given: msda_loc_delta) + the attention weights'
    (attw_c + 2) u A (attw_c of msda_prep_ref given; + 2: a reciprocal and a product for the divide).
    kernel: 'f32', 'fast', 'strip' or 'records'.  The records front end passes neither: its reference
    samples the decoded records.  The addressing class passes no attw_c: its softmax is exactly (1, 0, ...)."""
    A, ref = samp['A'], samp['out']
    # an f16 result below 2^-14 is subnormal: its rounding is absolute, F16_W_ABS, not relative -- the output
    # itself, and in the strip kernel each of the 64 packed-f16 multiply-adds behind an element
    b = OUT_ROUND[out_dtype] * ref.abs() + (F16_W_ABS if out_dtype == torch.float16 else 0.0)
    if kernel == 'f32':
        b = b + C_ACC_F32 * A
    elif kernel == 'fast':
        b = b + (C_ACC_F32 + F16_W) * A + F16_W_ABS * samp['V']
    else:
        nw = 2 if kernel == 'records' else 1
        b = b + (nw * F16_W + 8 * U32) * A + 16 * F16_W * samp['A_lvl'].sum(0) + nw * F16_W_ABS * samp['V'] + 64 * F16_W_ABS
    if locA is not None:
        b = b + (samp['G_lvl'] * msda_loc_delta({'locA': locA}, shapes).view(-1, 1, 1, 1)).sum(0)
    if attw_c is not None:
        B, Lq, M = attw_c.shape[:3]
        c = (attw_c.amax((3, 4)) + 2) * U32
        b = b + (c[..., None] * A.reshape(B, Lq, M, -1)).reshape(A.shape)
    return b + 1e-30


# ----------------------------------------------------------------------------------------------
# MSDA launch plans (csrc/msda_plan.h through kinet_msda_launch_plan), worked by hand from the rules
# ----------------------------------------------------------------------------------------------
# sizeof the device structs the LDS formulas count (msda_plan.h; msda.hip static_asserts them)
MSDA_LDS_LIMIT = 160 * 1024
MSDA_LEVELINFO, MSDA_TAP4, MSDA_TAP4D, MSDA_BWDTAP32, MSDA_BWDTAP64, MSDA_HTAP = 256, 32, 48, 40, 64, 32
MSDA_FUSED_GENERIC, MSDA_FUSED_FAST = 1 << 8, 2 << 8     # kinet_msda_fused_last_kernel: family << 8 | detail
MSDA_KEEP_LAST = -2                                       # the plain forward records no last kernel

# (element size, D, M) -> (vec, lanes per (query, head), queries per workgroup); qt 0 = refused
MSDA_CFG_CASES = [
    (4, 32, 8, (4, 8, 4)),
    (2, 36, 8, (4, 9, 3)), (4, 36, 8, (4, 9, 3)),
    (8, 32, 8, (2, 16, 2)),
    (4, 33, 8, (1, 33, 0)), (2, 33, 8, (1, 33, 0)),
]

# the level set of test_backward_list_kernel_vs_oracle
MSDA_BWD_LEVELS = ((20, 33), (10, 17), (5, 9), (3, 5))
MSDA_BWD_S = 890


def msda_plan_row(family, **f):
    """A full plan record: every field 0 but grid (1, 1, 1) and the ones named."""
    import kinet_amd.kernels as K
    row = dict.fromkeys(K.MSDA_PLAN_FIELDS, 0)
    row.update(family=family, grid_x=1, grid_y=1, grid_z=1, last=MSDA_KEEP_LAST)
    grid = f.pop('grid', None)
    if grid:
        row.update(zip(('grid_x', 'grid_y', 'grid_z'), tuple(grid) + (1,) * (3 - len(grid))))
    row.update(f)
    return row


def msda_list_lds(QP, LP, D, log2ns):
    """LevelInfo | keys, head, plist [2^log2ns] | npass[4] | cinfo (int2) + next per corner | G[QP][D] | taps"""
    return MSDA_LEVELINFO + 3 * (1 << log2ns) * 4 + 16 + QP * LP * 4 * (8 + 4) + QP * D * 4 + QP * LP * MSDA_HTAP


def _bwd_list(D, grid, block=256, QP=16, qc=16, log2ns=10, blocked=1, sp=2):
    return msda_plan_row('msda_bwd_list_kernel', vec=4, nj=(D + 15) // 16, sp=sp, grid=grid, block=block,
                         lds=msda_list_lds(QP, 16, D, log2ns), na=D // 4, QP=QP, qc=qc, log2ns=log2ns, blocked=blocked,
                         last=1)


def _bwd_direct(D, Lq):
    """f32, M = 8, L*P = 16: D = 32 -> 8 lanes x 4 queries; D = 36 -> 9 lanes padded to 16 x 2 queries, ALN."""
    lpq, qt = (8, 4) if D == 32 else (16, 2)
    return msda_plan_row('msda_bwd_kernel', vec=4, pow2=1, aln=int(D == 36), qt=qt, lpq=lpq, na=D // 4,
                         grid=(-(-Lq // qt), 2), block=256, lds=MSDA_LEVELINFO + qt * 8 * 16 * MSDA_BWDTAP32, last=0)


# (name, value dtype, D, Lq, tune (mode, log2_rows, queries per block, threads, queries per pass)) -> plan;
# N = 2, M = 8, L = P = 4, S = 890.  Blocked grid: ceil(S / QP) blocks + 1/8 + 2 per level.
MSDA_BWD_CASES = [
    ('auto', 'f32', 32, 890, (0, 0, 0, 0, 0), _bwd_list(32, (56 + 7 + 8, 2, 8))),
    ('auto Lq != S', 'f32', 32, 947, (0, 0, 0, 0, 0), _bwd_direct(32, 947)),
    ('auto D36 Lq != S', 'f32', 36, 947, (0, 0, 0, 0, 0), _bwd_direct(36, 947)),
    ('mode -1', 'f32', 32, 890, (-1, 0, 0, 0, 0), _bwd_direct(32, 890)),
    ('mode 1 Lq != S', 'f32', 32, 947, (1, 0, 0, 0, 0), _bwd_list(32, (60, 2, 8), blocked=0)),
    ('mode 2', 'f32', 32, 890, (2, 0, 0, 0, 0), _bwd_list(32, (56, 2, 8), blocked=0)),
    ('mode 3', 'f32', 32, 890, (3, 0, 0, 0, 0), _bwd_list(32, (71, 2, 8), sp=4)),
    # f64: 16 lanes x 2 doubles, 2 queries; f64 sums: never the list kernel, no ALN
    ('f64', 'f64', 32, 890, (0, 0, 0, 0, 0),
     msda_plan_row('msda_bwd_kernel', vec=2, pow2=1, qt=2, lpq=16, na=16, grid=(445, 2), block=256,
                   lds=MSDA_LEVELINFO + 2 * 8 * 16 * MSDA_BWDTAP64, last=0)),
    ('f64 mode 1', 'f64', 32, 890, (1, 0, 0, 0, 0),
     msda_plan_row('msda_bwd_kernel', vec=2, pow2=1, qt=2, lpq=16, na=16, grid=(445, 2), block=256,
                   lds=MSDA_LEVELINFO + 2 * 8 * 16 * MSDA_BWDTAP64, last=0)),
    # D = 80: nj = 5 > 4; 20 lanes padded to 32, one query per workgroup
    ('D80', 'f32', 80, 890, (0, 0, 0, 0, 0),
     msda_plan_row('msda_bwd_kernel', vec=4, pow2=1, qt=1, lpq=32, na=20, grid=(890, 2), block=256,
                   lds=MSDA_LEVELINFO + 8 * 16 * MSDA_BWDTAP32, last=0)),
]
# every (tune, extra queries) of test_backward_list_kernel_vs_oracle at D = 32 and 36
MSDA_BWD_TUNE_CASES = []
for _D in (32, 36):
    MSDA_BWD_TUNE_CASES += [
        ((0, 0, 0, 0, 0), 0, _D, _bwd_list(_D, (71, 2, 8))),
        ((1, 0, 0, 0, 0), 57, _D, _bwd_list(_D, (60, 2, 8), blocked=0)),
        ((1, 6, 32, 256, 0), 57, _D, _bwd_list(_D, (30, 2, 8), qc=32, log2ns=6, blocked=0)),
        ((1, 6, 64, 512, 16), 57, _D, _bwd_list(_D, (15, 2, 8), block=512, qc=64, log2ns=6, blocked=0)),
        # passes of 64 queries: ceil(890 / 64) = 14 blocks + 1 + 8
        ((1, 10, 512, 512, 64), 0, _D, _bwd_list(_D, (23, 2, 8), block=512, QP=64, qc=512)),
        ((2, 0, 0, 0, 0), 0, _D, _bwd_list(_D, (56, 2, 8), blocked=0)),
        ((0, 0, 0, 0, 0), 57, _D, _bwd_direct(_D, 947)),
        ((-1, 0, 0, 0, 0), 0, _D, _bwd_direct(_D, 890)),
        ((3, 0, 0, 0, 0), 0, _D, _bwd_list(_D, (71, 2, 8), sp=4)),
    ]


def _fused_fast(L, Lq, N, M, S, vss=256):
    MH = 2 if L == 4 else 4
    return msda_plan_row('msda_fused_fast_kernel', l=L, sg=MH, QT=16, MH=MH, grid=(-(-Lq // 16), N, -(-M // MH)),
                         block=64 * MH, lds=0, head_bytes=((S - 1) * vss + 32) * 2, last=MSDA_FUSED_FAST | L)


def _fused_generic(vec, lpq, LP, Lq, N, M):
    """one head per wave, 64 // lpq queries per wave, 4 waves; logits staged (4 B) unless L*P is a power of two"""
    QT = 64 // lpq
    pow2 = LP & (LP - 1) == 0 and LP <= 64
    return msda_plan_row('msda_fused_kernel', vec=vec, lpq=lpq, QT=QT, MH=4, grid=(-(-Lq // QT), N, -(-M // 4)),
                         block=256, lds=MSDA_LEVELINFO + 4 * QT * LP * (MSDA_TAP4 + (0 if pow2 else 4)),
                         last=MSDA_FUSED_GENERIC | vec)


MSDA_ALIGN_MSG = 'msda fused: value strides must keep 8-element vectors aligned'
MSDA_F16_MSG = ('msda fused: output dtype != value dtype or f16 offsets/logits need head_dim 32, '
                'L*P in {16, 32}, P = 4 and aligned strides')
# (name, dict(value, out, offlog dtypes, D, L, P, S, Lq, N, M, strides (sb, ss, sm), align)) -> plan, or the
# refusal's message.  Row-major strides of (N, S, 8, 32): (S * 256, 256, 32).
_FB = dict(value='bf16', out='bf16', offlog='f32', D=32, L=4, P=4, S=890, Lq=947, N=2, M=8, strides=(890 * 256, 256, 32),
           align=0)
MSDA_FUSED_CASES = [
    ('fast L4', _FB, _fused_fast(4, 947, 2, 8, 890)),
    ('fast L4 f16 -> bf16, f16 offsets', dict(_FB, value='f16', offlog='f16'), _fused_fast(4, 947, 2, 8, 890)),
    ('fast L4 M5', dict(_FB, M=5, strides=(890 * 160, 160, 32)), _fused_fast(4, 947, 2, 5, 890, 160)),
    ('fast L8', dict(_FB, L=8), _fused_fast(8, 947, 2, 8, 890)),
    ('fast L8 M5', dict(_FB, L=8, M=5, strides=(890 * 160, 160, 32)), _fused_fast(8, 947, 2, 5, 890, 160)),
    ('fast head-major', dict(_FB, strides=(890 * 32, 32, 2 * 890 * 32)), _fused_fast(4, 947, 2, 8, 890, 32)),
    # one condition of the fast kernel broken at a time: the generic kernel (8 bf16 per lane, 4 lanes, 16 queries
    # per wave) -- which itself needs 8-element alignment
    ('pixel stride % 8', dict(_FB, strides=(890 * 260, 260, 32)), MSDA_ALIGN_MSG),
    ('batch stride % 8', dict(_FB, strides=(890 * 256 + 4, 256, 32)), MSDA_ALIGN_MSG),
    ('head stride % 8', dict(_FB, strides=(890 * 256, 256, 36)), MSDA_ALIGN_MSG),
    ('pointer % 16', dict(_FB, align=8), MSDA_ALIGN_MSG),
    ('head_bytes 2^31 + 64', dict(_FB, S=(1 << 22) + 1, strides=(((1 << 22) + 1) * 256, 256, 32)),
     _fused_generic(8, 4, 16, 947, 2, 8)),
    ('head_bytes 2^31 - 448', dict(_FB, S=1 << 22, strides=((1 << 22) * 256, 256, 32)), _fused_fast(4, 947, 2, 8, 1 << 22)),
    ('P = 2', dict(_FB, P=2), _fused_generic(8, 4, 8, 947, 2, 8)),
    ('L = 3, P = 5', dict(_FB, L=3, P=5), _fused_generic(8, 4, 15, 947, 2, 8)),
    ('D = 36', dict(_FB, D=36, strides=(890 * 288, 288, 36)), _fused_generic(4, 9, 16, 947, 2, 8)),
    ('f32', dict(_FB, value='f32', out='f32'), _fused_generic(4, 8, 16, 947, 2, 8)),
    ('f16 offsets, D = 36', dict(_FB, D=36, strides=(890 * 288, 288, 36), offlog='f16'), MSDA_F16_MSG),
    ('f16 -> bf16, P = 2', dict(_FB, value='f16', P=2), MSDA_F16_MSG),
    ('empty', dict(_FB, Lq=0), msda_plan_row('none', last=-1)),
]

# plain forward: (value dtype, D, Lq) -> plan; N = 2, M = 8, L = P = 4
MSDA_FWD_CASES = [
    ('f32', 32, 947, msda_plan_row('msda_fwd_kernel', vec=4, qt=4, lpq=8, grid=(237, 2), block=256,
                                    lds=MSDA_LEVELINFO + 4 * 8 * 16 * MSDA_TAP4)),
    ('bf16', 36, 947, msda_plan_row('msda_fwd_kernel', vec=4, qt=3, lpq=9, grid=(316, 2), block=256,
                                     lds=MSDA_LEVELINFO + 3 * 8 * 16 * MSDA_TAP4)),
    ('f64', 32, 947, msda_plan_row('msda_fwd_kernel', vec=2, qt=2, lpq=16, grid=(474, 2), block=256,
                                    lds=MSDA_LEVELINFO + 2 * 8 * 16 * MSDA_TAP4D)),
    ('f32', 32, 0, msda_plan_row('none')),
]


# ----------------------------------------------------------------------------------------------
# Fused FFN / bottleneck-pair launch plans (csrc/ffn_plan.h through kinet_ffn_launch_plan), worked by
# hand from the rules.  256 compute units.
# ----------------------------------------------------------------------------------------------
FFN_LDS_LIMIT = 160 * 1024
# the bits of kinet_ffn_set_debug (FfnDebug, csrc/ffn_plan.h)
FFN_DBG_NO_DMA, FFN_DBG_4W_RT2, FFN_DBG_8W_RT1, FFN_DBG_PAIR64_RING = 1, 2, 8, 16
FFN_DBG_ATTN_RV1, FFN_DBG_PAIR_RT1, FFN_DBG_PAIR_RT2, FFN_DBG_DS_RT2 = 64, 128, 256, 512

# the table of instantiations: name -> (waves, rows per row tile, row tiles a workgroup works on, workgroups
# per CU, LDS bytes).  LDS: parameters + ring slots x (32-unit chunk of 2 D/32 + D/16 KiB [+ 64 B per row of
# residual]), or 8 chunks of resident fragments + parameters
FFN_KERNELS = {
    'ffn_fused_kernel<256, 2, 4>': (4, 128, 1, 1, (2048 + 3 * 256) * 4 + 4 * 32 * 1024),
    'ffn_fused_kernel<256, 1, 8>': (8, 128, 1, 1, (2048 + 3 * 256) * 4 + 4 * 32 * 1024),
    'ffn_fused_kernel<256, 1, 4>': (4, 64, 1, 1, (2048 + 3 * 256) * 4 + 4 * 32 * 1024),
    'ffn_fused_kernel<288, 2, 4>': (4, 128, 1, 1, (2048 + 3 * 288) * 4 + 4 * 36 * 1024),
    'ffn_fused_kernel<288, 1, 4>': (4, 64, 1, 1, (2048 + 3 * 288) * 4 + 4 * 36 * 1024),
    'ffn_fused_rt2_kernel<256>': (8, 256, 1, 1, (2048 + 3 * 256) * 4 + 3 * 32 * 1024),
    'ffn_fused_rt2_kernel<256, true>': (8, 256, 1, 1, (2048 + 6 * 256) * 4 + 3 * 32 * 1024),
    'ffn_fused_rt2_kernel<256, true, 1>': (8, 256, 1, 1, (2048 + 6 * 256) * 4 + 3 * 32 * 1024),
    'bneck_pair_kernel<64, 2, 8>': (8, 256, 1, 2, 5 * 64 * 4 + 3 * (8 * 1024 + 256 * 64)),
    'bneck_pair_kernel<128, 1, 8>': (8, 128, 1, 1, 5 * 128 * 4 + 3 * (16 * 1024 + 128 * 64)),
    'bneck_pair_kernel<128, 2, 8>': (8, 256, 1, 1, 5 * 128 * 4 + 3 * (16 * 1024 + 256 * 64)),
    'bneck_pair_kernel<256, 1, 8>': (8, 128, 1, 1, 5 * 256 * 4 + 3 * (32 * 1024 + 128 * 64)),
    'bneck_pair_kernel<256, 2, 8>': (8, 256, 1, 1, 5 * 256 * 4 + 3 * (32 * 1024 + 256 * 64)),
    'bneck64_kernel<128, 16>': (16, 16, 16, 1, 8 * 12 * 1024 + (256 + 128) * 4),
    'bneck64_kernel<64, 8>': (8, 16, 8, 2, 8 * 8 * 1024 + (256 + 64) * 4),
    'bneck64_ds_kernel<1>': (16, 16, 16, 1, 8 * 12 * 1024 + (256 + 64) * 4),
    'bneck64_ds_kernel<2>': (16, 32, 16, 1, 8 * 12 * 1024 + (256 + 64) * 4),
}
_F24, _F18, _F14 = 'ffn_fused_kernel<%d, 2, 4>', 'ffn_fused_kernel<%d, 1, 8>', 'ffn_fused_kernel<%d, 1, 4>'
_RT2, _PRE0, _PRE1 = 'ffn_fused_rt2_kernel<256>', 'ffn_fused_rt2_kernel<256, true>', 'ffn_fused_rt2_kernel<256, true, 1>'
_PAIR = 'bneck_pair_kernel<%d, %d, 8>'
_B64, _B128, _DS1, _DS2 = 'bneck64_kernel<64, 8>', 'bneck64_kernel<128, 16>', 'bneck64_ds_kernel<1>', 'bneck64_ds_kernel<2>'
FFN_MSG_D = 'ffn_fused: D must be 256 or 288 (got %d)'
FFN_MSG_ATTN_288 = 'attn_out_ffn_fused: D = 288 is not supported (Wo does not fill whole ring chunks); D must be 256'
FFN_MSG_ATTN_D = 'attn_out_ffn_fused: D must be 256 (got %d)'
FFN_MSG_PAIR_D = 'bottleneck_pair: D must be 64, 128 or 256 (got %d)'
FFN_MSG_PAIR_DB = 'bottleneck_pair: DB must be D, or 128 at D = 64 (got D=%d DB=%d)'
FFN_MSG_DS_D = 'bottleneck_pair_ds: D must be 64 (got %d)'
FFN_MSG_DS_DB = 'bottleneck_pair_ds: DB must be 64 (got %d)'

# (kind, M, D, DB, debug bits, solo) -> (kernel, row tiles, grid), or the refusal's message; an eighth field is the
# calling thread's kinet_ffn_grid_cap (none: 0)
FFN_PLAN_CASES = [
    # kinet_ffn_fused: 4 waves x 16 rows below 16384 rows, whatever the knobs
    ('ffn', 1, 256, 256, 0, 0, (_F14 % 256, 1, 1)),
    ('ffn', 16383, 256, 256, 0, 0, (_F14 % 256, 256, 256)),
    ('ffn', 16383, 256, 256, 2, 0, (_F14 % 256, 256, 256)),
    ('ffn', 16383, 256, 256, 8, 0, (_F14 % 256, 256, 256)),
    ('ffn', 16383, 256, 256, 2 | 8, 0, (_F14 % 256, 256, 256)),
    ('ffn', 16383, 288, 288, 0, 0, (_F14 % 288, 256, 256)),
    # from 16384: 8 waves x 32 rows; knob 2 the 4-wave x 32-row tile, knob 8 the 8-wave x 16-row tile, 2 before 8
    ('ffn', 16384, 256, 256, 0, 0, (_RT2, 64, 64)),
    ('ffn', 16384, 256, 256, 1, 0, (_RT2, 64, 64)),
    ('ffn', 16384, 256, 256, 2, 0, (_F24 % 256, 128, 128)),
    ('ffn', 16384, 256, 256, 8, 0, (_F18 % 256, 128, 128)),
    ('ffn', 16384, 256, 256, 2 | 8, 0, (_F24 % 256, 128, 128)),
    ('ffn', 355568, 256, 256, 0, 0, (_RT2, 1389, 256)),
    ('ffn', 355568, 256, 256, 2, 0, (_F24 % 256, 2778, 256)),
    # D = 288 (36 fragments per chunk: no whole rounds of 8 waves): the 4-wave x 32-row tile under every knob
    ('ffn', 16384, 288, 288, 0, 0, (_F24 % 288, 128, 128)),
    ('ffn', 16384, 288, 288, 2, 0, (_F24 % 288, 128, 128)),
    ('ffn', 16384, 288, 288, 8, 0, (_F24 % 288, 128, 128)),
    ('ffn', 16384, 128, 128, 0, 0, FFN_MSG_D % 128),
    # kinet_attn_out_ffn_fused: the 8-wave x 32-row tile at every M; knob 64 = RV 1
    ('attn_out_ffn', 5, 256, 256, 0, 0, (_PRE0, 1, 1)),
    ('attn_out_ffn', 16384, 256, 256, 0, 0, (_PRE0, 64, 64)),
    ('attn_out_ffn', 16384, 256, 256, 64, 0, (_PRE1, 64, 64)),
    ('attn_out_ffn', 16384, 256, 256, 2 | 8, 0, (_PRE0, 64, 64)),
    ('attn_out_ffn', 355568, 256, 256, 0, 0, (_PRE0, 1389, 256)),
    ('attn_out_ffn', 16384, 288, 288, 0, 0, FFN_MSG_ATTN_288),
    ('attn_out_ffn', 16384, 128, 128, 0, 0, FFN_MSG_ATTN_D % 128),
    # kinet_bottleneck_pair at D = 128 / 256.  M = 32640: 128 2-tile tiles fill half a round of 256 CUs, 255 1-tile
    # tiles 0.996 of one: the 1-tile grid with one batch in flight only
    ('pair', 32640, 128, 128, 0, 0, (_PAIR % (128, 2), 128, 128)),
    ('pair', 32640, 128, 128, 0, 1, (_PAIR % (128, 1), 255, 255)),
    ('pair', 32640, 256, 256, 0, 0, (_PAIR % (256, 2), 128, 128)),
    ('pair', 32640, 256, 256, 0, 1, (_PAIR % (256, 1), 255, 255)),
    # e1 <= 1.5 e2 with solo on: both fill whole rounds (65536); 460 / 512 vs 919 / 1024 (117600)
    ('pair', 65536, 128, 128, 0, 1, (_PAIR % (128, 2), 256, 256)),
    ('pair', 117600, 256, 256, 0, 1, (_PAIR % (256, 2), 460, 256)),
    # the rule's edge: 1 vs 1 tile (128 rows), 2 vs 1 (129), 3 vs 2 = exactly 1.5 (300), 4 vs 2 (400)
    ('pair', 128, 256, 256, 0, 1, (_PAIR % (256, 2), 1, 1)),
    ('pair', 129, 256, 256, 0, 1, (_PAIR % (256, 1), 2, 2)),
    ('pair', 300, 256, 256, 0, 1, (_PAIR % (256, 2), 2, 2)),
    ('pair', 400, 256, 256, 0, 1, (_PAIR % (256, 1), 4, 4)),
    # knob 128 before knob 256 before the solo rule
    ('pair', 32640, 128, 128, 128, 0, (_PAIR % (128, 1), 255, 255)),
    ('pair', 32640, 128, 128, 256, 1, (_PAIR % (128, 2), 128, 128)),
    ('pair', 32640, 128, 128, 128 | 256, 0, (_PAIR % (128, 1), 255, 255)),
    ('pair', 65536, 256, 256, 128, 1, (_PAIR % (256, 1), 512, 256)),
    # D = 64: resident weights, a 16-row tile per wave, 2 x 8 waves per CU; knob 16 the ring kernel (2 per CU);
    # DB = 128 first: 16 waves, one workgroup per CU, no knob
    ('pair', 1000, 64, 64, 0, 0, (_B64, 63, 8)),
    ('pair', 1000, 64, 64, 16, 0, (_PAIR % (64, 2), 4, 4)),
    ('pair', 1068800, 64, 64, 0, 0, (_B64, 66800, 512)),
    ('pair', 1068800, 64, 64, 16, 0, (_PAIR % (64, 2), 4175, 512)),
    ('pair', 1000, 64, 128, 0, 0, (_B128, 63, 4)),
    ('pair', 1000, 64, 128, 16, 0, (_B128, 63, 4)),
    ('pair', 1068800, 64, 128, 0, 0, (_B128, 66800, 256)),
    ('pair', 1000, 128, 64, 0, 0, FFN_MSG_PAIR_DB % (128, 64)),
    ('pair', 1000, 64, 256, 0, 0, FFN_MSG_PAIR_DB % (64, 256)),
    ('pair', 1000, 96, 96, 0, 0, FFN_MSG_PAIR_D % 96),
    # kinet_bottleneck_pair_ds: knob 512 = two 16-row tiles per wave
    ('pair_ds', 1000, 64, 64, 0, 0, (_DS1, 63, 4)),
    ('pair_ds', 1000, 64, 64, 512, 0, (_DS2, 32, 2)),
    ('pair_ds', 1068800, 64, 64, 0, 0, (_DS1, 66800, 256)),
    ('pair_ds', 1068800, 64, 64, 512, 0, (_DS2, 33400, 256)),
    ('pair_ds', 1000, 128, 128, 0, 0, FFN_MSG_DS_D % 128),
    ('pair_ds', 1000, 64, 128, 0, 0, FFN_MSG_DS_DB % 128),
    # kinet_ffn_grid_cap: the grid is min(workgroups that cover the tiles, CUs x workgroups per CU, the cap); the
    # kernel and the tiles do not move.  1389 tiles on 256 CUs under caps 100 and 300; 256 tiles under cap 1
    ('ffn', 355568, 256, 256, 0, 0, (_RT2, 1389, 100), 100),
    ('ffn', 355568, 256, 256, 0, 0, (_RT2, 1389, 256), 300),
    ('ffn', 16383, 256, 256, 0, 0, (_F14 % 256, 256, 1), 1),
    ('ffn', 16384, 288, 288, 0, 0, (_F24 % 288, 128, 127), 127),
    ('attn_out_ffn', 5, 256, 256, 0, 0, (_PRE0, 1, 1), 4),
    ('attn_out_ffn', 355568, 256, 256, 64, 0, (_PRE1, 1389, 255), 255),
    # the solo rule looks at the CUs, not at the cap: 255 one-tile tiles still win, then the cap bounds them
    ('pair', 32640, 128, 128, 0, 1, (_PAIR % (128, 1), 255, 16), 16),
    # resident weights: 63 tiles in 8 workgroups of 8 waves (4 of 16 waves); the cap counts workgroups, not tiles
    ('pair', 1000, 64, 64, 0, 0, (_B64, 63, 8), 8),
    ('pair', 1000, 64, 64, 0, 0, (_B64, 63, 7), 7),
    ('pair', 1068800, 64, 64, 0, 0, (_B64, 66800, 3), 3),
    ('pair', 1000, 64, 128, 0, 0, (_B128, 63, 2), 2),
    ('pair_ds', 1000, 64, 64, 512, 0, (_DS2, 32, 1), 1),
    ('pair_ds', 1068800, 64, 64, 0, 0, (_DS1, 66800, 256), 257),
    ('ffn', 16384, 128, 128, 0, 0, FFN_MSG_D % 128, 2),
]

# packed-weight layout (ffn_pack_src): (kind, D, F, DB, packed index) -> (source matrix, row, column).  Index =
# ((chunk * fragments per chunk + fragment) * 64 + lane) * 8 + j, lane = 16 g + c; the formulas of the comment in
# csrc/ffn_plan.h, by hand
FFN_PACK_CASES = [
    ('ffn', 256, 64, 256, 0, (0, 0, 0)),
    # chunk 1, fragment 9 = W1 (h-tile 1, k-step 1), lane 37 = (2, 5), j 5: row 32 + 16 + 5, column 32 + 16 + 5
    ('ffn', 256, 64, 256, (1 * 32 + 9) * 512 + 37 * 8 + 5, (0, 53, 53)),
    # chunk 0, fragment 16 + 3 = W2 tile 3, lane 22 = (1, 6), j 6: row sigma(3, 6) = 32 + 8 + 4 + 2, hidden 16 + 4 + 2
    ('ffn', 256, 64, 256, 19 * 512 + 22 * 8 + 6, (1, 46, 22)),
    # Wo fragment 37 = (k-step 2, tile 5), lane 63 = (3, 15), j 7: row sigma(5, 15) = 64 + 24 + 4 + 3, column 64 + 24 + 7
    ('attn_out_ffn', 256, 64, 256, 37 * 512 + 63 * 8 + 7, (0, 95, 95)),
    ('attn_out_ffn', 256, 64, 256, 256 * 256 + 19 * 512 + 22 * 8 + 6, (2, 46, 22)),
    # D = 64 -> DB = 128: 4 + 8 fragments per chunk.  chunk 3, fragment 2 = W3 (h-tile 1, k-step 0), lane 17 = (1, 1), j 1
    ('pair', 64, 256, 128, (3 * 12 + 2) * 512 + 17 * 8 + 1, (0, 113, 9)),
    # chunk 7, fragment 4 + 7 = W1 tile 7, lane 40 = (2, 8), j 3: row sigma(7, 8) = 96 + 16 + 4, hidden 224 + 8 + 3
    ('pair', 64, 256, 128, (7 * 12 + 11) * 512 + 40 * 8 + 3, (1, 116, 235)),
    # ds: W3, W_ds, W1 = 4 + 4 + 4 fragments.  chunk 1, fragment 6 = W_ds (h-tile 1, k-step 0), lane 5 = (0, 5), j 2
    ('pair_ds', 64, 256, 64, (1 * 12 + 6) * 512 + 5 * 8 + 2, (1, 53, 2)),
    # chunk 0, fragment 9 = W1 tile 1, lane 48 = (3, 0), j 4: row sigma(1, 0) = 4, hidden 16 + 12
    ('pair_ds', 64, 256, 64, 9 * 512 + 48 * 8 + 4, (2, 4, 28)),
    # D = 288: 18 + 18 fragments.  chunk 1, fragment 17 = W1 (h-tile 1, k-step 8), lane 31 = (1, 15), j 0
    ('ffn', 288, 64, 288, (36 + 17) * 512 + 31 * 8, (0, 63, 264)),
    # chunk 0, fragment 35 = W2 tile 17, lane 15 = (0, 15), j 7: row sigma(17, 15) = 256 + 24 + 4 + 3, hidden 16 + 3
    ('ffn', 288, 64, 288, 35 * 512 + 15 * 8 + 7, (1, 287, 19)),
]
# (kind, D, F, DB) the models pack, plus D = 288 and the shapes of tests/test_ffn_pack_gpu.py
FFN_PACK_SHAPES = [
    ('ffn', 256, 1024, 256), ('ffn', 256, 2048, 256), ('ffn', 288, 1024, 288), ('attn_out_ffn', 256, 1024, 256),
    ('attn_out_ffn', 288, 64, 288), ('pair', 64, 256, 64), ('pair', 64, 256, 128), ('pair', 128, 512, 128),
    ('pair', 256, 1024, 256), ('pair', 288, 64, 288), ('pair_ds', 64, 256, 64), ('ffn', 64, 256, 64), ('ffn', 256, 64, 256),
]


def ffn_pack_shapes(kind, D, F, DB):
    """Shapes of a pack kind's source matrices, in the pack call's argument order."""
    return {'ffn': [(F, D), (D, F)], 'attn_out_ffn': [(D, D), (F, D), (D, F)], 'pair': [(F, D), (DB, F)],
            'pair_ds': [(F, D), (F, D), (DB, F)]}[kind]


# ----------------------------------------------------------------------------------------------
# Direct tests of the fused FFN / bottleneck-pair kernels (csrc/ffn.hip; tests/test_ffn_direct_gpu.py).
#
# The table: (entry point, D, F, DB, M, debug bits, solo, kernel, rows per row tile, {grid cap: grid}),
# written down from the rules of csrc/ffn_plan.h for 256 compute units; test_ffn_plan_cpu.py holds every
# row, under every cap, against kinet_ffn_launch_plan.
#   ring kernels the planner serves at any M: five row tiles, the last ragged (M = 5 rows - 5); cap 0 =
#     one tile per workgroup, 1 = one workgroup walks all five, 2 = 3 / 2 tiles, 4 = one workgroup with
#     two tiles beside three with one;
#   the four kernels kinet_ffn_fused takes from 16384 rows: M = 16635 = 65 tiles of 256 rows or 130 of
#     128, ragged; caps 0, 1, 3, tiles - 1;
#   resident weights (a 16 rt-row tile per wave): M = rows (2 waves + 3) - 5 -> 2 waves + 3 tiles in 3
#     workgroups, the last one with idle waves and a ragged tile; under cap 1 every wave walks two or
#     three tiles (the refill of the residual registers), under cap 2 one or two.
# F (FFN entry points): 32, 64, 160 = 1, 2, 5 hidden chunks (5: a multiple of neither ring depth), and
# 2048 = FFN_MAX_F on the kernels that run at few rows; the pairs take F = 4 D only.
# ----------------------------------------------------------------------------------------------
FFN_BIG_ROWS = 16635
_CAPS5 = {0: 5, 1: 1, 2: 2, 4: 4}
_CAPS65, _CAPS130 = {0: 65, 1: 1, 3: 3, 64: 64}, {0: 130, 1: 1, 3: 3, 129: 129}
_CAPS_RES = {0: 3, 1: 1, 2: 2}
FFN_DIRECT_CASES = (
    [('ffn', 256, F_, 256, 315, 0, 0, _F14 % 256, 64, _CAPS5) for F_ in (32, 64, 160, 2048)]
    + [('ffn', 288, F_, 288, 315, 0, 0, _F14 % 288, 64, _CAPS5) for F_ in (32, 64, 160, 2048)]
    + [('attn_out_ffn', 256, F_, 256, 1275, 0, 0, _PRE0, 256, _CAPS5) for F_ in (32, 64, 160, 2048)]
    + [('attn_out_ffn', 256, F_, 256, 1275, 64, 0, _PRE1, 256, _CAPS5) for F_ in (32, 64, 160, 2048)]
    + [('ffn', 256, F_, 256, FFN_BIG_ROWS, 0, 0, _RT2, 256, _CAPS65) for F_ in (32, 64, 160)]
    + [('ffn', 256, F_, 256, FFN_BIG_ROWS, 2, 0, _F24 % 256, 128, _CAPS130) for F_ in (32, 64, 160)]
    + [('ffn', 256, F_, 256, FFN_BIG_ROWS, 8, 0, _F18 % 256, 128, _CAPS130) for F_ in (32, 64, 160)]
    + [('ffn', 288, F_, 288, FFN_BIG_ROWS, 0, 0, _F24 % 288, 128, _CAPS130) for F_ in (32, 64, 160)]
    + [('pair', 64, 256, 64, 1275, 16, 0, _PAIR % (64, 2), 256, _CAPS5),
       ('pair', 128, 512, 128, 635, 128, 0, _PAIR % (128, 1), 128, _CAPS5),
       ('pair', 256, 1024, 256, 635, 128, 0, _PAIR % (256, 1), 128, _CAPS5),
       ('pair', 128, 512, 128, 1275, 256, 0, _PAIR % (128, 2), 256, _CAPS5),
       ('pair', 256, 1024, 256, 1275, 256, 0, _PAIR % (256, 2), 256, _CAPS5),
       # 19 tiles over 8 waves, 35 over 16: 3 workgroups
       ('pair', 64, 256, 64, 16 * 19 - 5, 0, 0, _B64, 16, _CAPS_RES),
       ('pair', 64, 256, 128, 16 * 35 - 5, 0, 0, _B128, 16, _CAPS_RES),
       ('pair_ds', 64, 256, 64, 16 * 35 - 5, 0, 0, _DS1, 16, _CAPS_RES),
       ('pair_ds', 64, 256, 64, 32 * 35 - 5, 512, 0, _DS2, 32, _CAPS_RES)])


def ffn_case_id(case):
    return '-'.join(map(str, case[:7]))


def ffn_direct_ld(case):
    """Row strides of a case's operands: every X (and A) D + 8, the FFN entries' Y D + 16, the attention residual
    D + 24, the downsample pair's block input 72."""
    D = case[1]
    return dict(ldx=D + 8, ldy=D + 16, lda=D + 8, ldr=D + 24, ldx0=72)


# --- the references: plain f64, stage by stage; `drop` = (GEMM name, row, output column, k) takes that one
# product out of that GEMM's sum (the probes of test_direct_refs_cpu.py) ---
def rnd(v, dtype):
    """v rounded to dtype, in f64."""
    return v.to(dtype).double()


def _mm(a, b, drop, name):
    """(a (M, K) @ b (N, K)^T, |a| @ |b|^T)."""
    acc = a @ b.T
    if drop is not None and drop[0] == name:
        _, m, n, k = drop
        acc[m, n] = acc[m, n] - a[m, k] * b[n, k]
    return acc, a.abs() @ b.abs().T


def ffn_ref(x, W1, b1, W2, b2, ln, dtype, drop=None):
    """kinet_ffn_fused on x (M, D) holding values of dtype: h = relu(x W1^T + b1) rounded once to dtype, pre = x +
    h W2^T + b2, y = LayerNorm(pre) for ln = (gamma, beta, eps), else pre (the caller rounds the output).  Also the
    majorants of ffn_generic_bound: absA = |x| @ |W1|^T, majA = |acc| + |b1|, majB = |x| + |acc| + |b2|."""
    x, W1, b1, W2, b2 = (t.double() for t in (x, W1, b1, W2, b2))
    accA, absA = _mm(x, W1, drop, 'W1')
    h = rnd((accA + b1).clamp(min=0), dtype)
    accB, _ = _mm(h, W2, drop, 'W2')
    pre = x + accB + b2
    out = dict(x=x, h=h, pre=pre, absA=absA, majA=accA.abs() + b1.abs(), majB=x.abs() + accB.abs() + b2.abs())
    out['y'] = ln_epilogue_ref(pre, ln[0], ln[1], ln[2])['y'] if ln is not None else pre
    return out


def attn_out_ffn_ref(A, R, Wo, bo, ln1, W1, b1, W2, b2, ln2, dtype, drop=None):
    """kinet_attn_out_ffn_fused: x = LN1(R + A Wo^T + bo) rounded once to dtype (ln1 = (gamma, beta, eps)), then
    ffn_ref on that x.  pre1 / x64: the first LayerNorm's input / unrounded output; absO, majO its GEMM's majorants."""
    A, R, Wo, bo = (t.double() for t in (A, R, Wo, bo))
    accO, absO = _mm(A, Wo, drop, 'Wo')
    pre1 = R + accO + bo
    l1 = ln_epilogue_ref(pre1, ln1[0], ln1[1], ln1[2])
    out = ffn_ref(rnd(l1['y'], dtype), W1, b1, W2, b2, ln2, dtype, drop)
    out.update(pre1=pre1, x64=l1['y'], ln1=l1, absO=absO, majO=R.abs() + accO.abs() + bo.abs())
    return out


def scaled_rows(W, s, dtype):
    """A bottleneck pack's weight rows: the f32 weight times its f32 scale (one f32 rounding), rounded once to dtype."""
    return (W.float() * s.float().reshape(-1, 1)).to(dtype).double()


def pair_ref(X, R, W3, s3, b3, W1, s1, b1, dtype, drop=None):
    """kinet_bottleneck_pair: Y = relu(X (s3 W3)^T + b3 + R) rounded once (preY: before the rounding), T = relu(Y
    (s1 W1)^T + b1) from that rounded Y (preT likewise); each weight row scaled, then rounded once, as the pack does."""
    X, R, b3, b1 = (t.double() for t in (X, R, b3, b1))
    W3s, W1s = scaled_rows(W3, s3, dtype), scaled_rows(W1, s1, dtype)
    accA, absA = _mm(X, W3s, drop, 'W3')
    preY = (accA + b3 + R).clamp(min=0)
    return _pair_tail(preY, absA, accA.abs() + b3.abs() + R.abs(), W1s, b1, dtype, drop)


def pair_ds_ref(X, X0, W3, Wds, s3, sds, b3ds, W1, s1, b1, dtype, drop=None):
    """kinet_bottleneck_pair_ds: as pair_ref with Y = relu(X (s3 W3)^T + X0 (s_ds W_ds)^T + b3ds)."""
    X, X0, b3ds, b1 = (t.double() for t in (X, X0, b3ds, b1))
    W3s, Wdss, W1s = scaled_rows(W3, s3, dtype), scaled_rows(Wds, sds, dtype), scaled_rows(W1, s1, dtype)
    acc3, abs3 = _mm(X, W3s, drop, 'W3')
    accd, absd = _mm(X0, Wdss, drop, 'Wds')
    preY = (acc3 + accd + b3ds).clamp(min=0)
    return _pair_tail(preY, abs3 + absd, acc3.abs() + accd.abs() + b3ds.abs(), W1s, b1, dtype, drop)


def _pair_tail(preY, absA, majA, W1s, b1, dtype, drop):
    Y = rnd(preY, dtype)
    accB, _ = _mm(Y, W1s, drop, 'W1')
    return dict(preY=preY, Y=Y, preT=(accB + b1).clamp(min=0), absA=absA, majA=majA, majB=accB.abs() + b1.abs(), W1s=W1s)


# --- the generic class's bound ---
# u = U32, r = OUT_ROUND[dtype]; every product of two 16-bit values is exact in f32.
#   phase A, as gemm_generic_bound: K1 exact products summed in f32 in any order, then the bias (and the
#     residual) added:  errA = 1.01 (K1 + 64) u absA + 4 u majA  [+ dx @ |W1|^T where the operand itself is off
#     by dx: the attention entry's x];
#   the hidden: the kernel rounds its own f32 value, the reference its f64 one; |rd(p) - rd(q)| <= |p - q| +
#     r |p| + r |q| and relu does not widen |p - q|:  dh = (1 + r) errA + 2 r h, h the reference's rounded hidden;
#   phase B: that difference through |W2|, plus the accumulation of the kernel's own hidden (at most h + dh):
#     errB = dh @ |W2|^T + 1.01 (K2 + 64) u ((h + dh) @ |W2|^T);
#   the epilogue's additions (residual, bias; relu is exact): 4 u majB  [+ dx on the residual];
#   the output: rd(p) against the unrounded reference q: (1 + r) E + r |q| -- or, with the LayerNorm on,
#     ln_propagate(E) + the LayerNorm epilogue's own bound (ffn_ln_tol).
def ffn_generic_bound(absA, majA, h, W2abs, majB, K1, K2, dtype, dxA=None, dxres=None):
    """The bound E on |kernel's f32 value before the output rounding - the reference's| per element, and dh."""
    r = OUT_ROUND[dtype]
    errA = 1.01 * (K1 + 64) * U32 * absA + 4 * U32 * majA
    if dxA is not None:
        errA = errA + (1 + 1.01 * (K1 + 64) * U32) * dxA     # the kernel sums |x| + dx
    dh = (1 + r) * errA + 2 * r * h.abs()
    E = dh @ W2abs.T + 1.01 * (K2 + 64) * U32 * ((h.abs() + dh) @ W2abs.T) + 4 * U32 * majB
    if dxres is not None:
        E = E + dxres
    return E, dh


def out_round_bound(E, ref, dtype):
    return (1 + OUT_ROUND[dtype]) * E + OUT_ROUND[dtype] * ref.abs() + 1e-30


def ln_propagate(E, v, gamma, eps):
    """|LN(v') - LN(v)| for |v' - v| <= E elementwise, rigorously: the centred value moves by dc = E + mean E;
    the variance by at most dvar = mean(2 |c| dc + dc^2); rstd is decreasing and convex in the variance, so it moves
    by at most drs = (var + eps - dvar)^-1/2 - (var + eps)^-1/2; then |gamma| (dc (rstd + drs) + |c| drs)."""
    v = v.double()
    c = v - v.mean(-1, keepdim=True)
    dc = E + E.mean(-1, keepdim=True)
    var = (c * c).mean(-1, keepdim=True) + eps32(eps)
    dvar = (2 * c.abs() * dc + dc * dc).mean(-1, keepdim=True)
    assert (dvar < var).all()
    drs = (var - dvar).rsqrt() - var.rsqrt()
    return gamma.double().abs() * (dc * (var.rsqrt() + drs) + c.abs() * drs)


def ffn_ln_tol(pre, ln, dtype):
    """test_ln_epilogue_direct_gpu.py's bound on a fused LayerNorm epilogue's output (rw_ln_check): one rounding of
    the 16-bit output + 4x the error of torch's CPU f32 layer_norm of the same pre-activation.  (y64, tol)."""
    y, t = ln_epilogue_yardstick(pre.cpu(), ln[0].cpu(), ln[1].cpu(), ln[2])
    return y, OUT_ROUND[dtype] * y.abs() + 4 * t


# --- operands ---
def sparse_w(shape, q, g, unit=0.5):
    """+-unit with probability q each, +-2 unit with q / 4 each (exact_w's shape: var = 4 q unit^2); then one +-unit
    into every aligned 4-row x 32-column block and every column that came out empty.  Every 1-KiB fragment of the
    packed streams is four such blocks (16 rows of 4 aligned groups, 32 aligned columns: ffn_pack_src)."""
    u = torch.rand(shape, generator=g)
    w = torch.zeros(shape)
    for lo, hi, v in ((0, q, 1), (q, 2 * q, -1), (2 * q, 2.25 * q, 2), (2.25 * q, 2.5 * q, -2)):
        w[(u >= lo) & (u < hi)] = v
    R_, C_ = shape
    blocks = (w != 0).view(R_ // 4, 4, C_ // 32, 32).sum((1, 3)) == 0
    bi, bj = blocks.nonzero(as_tuple=True)
    if bi.numel():
        rr = 4 * bi + torch.randint(0, 4, bi.shape, generator=g)
        cc = 32 * bj + torch.randint(0, 32, bi.shape, generator=g)
        w[rr, cc] = torch.randint(0, 2, bi.shape, generator=g).float() * 2 - 1
    cols = ((w != 0).sum(0) == 0).nonzero().flatten()
    if cols.numel():
        w[torch.randint(0, R_, cols.shape, generator=g), cols] = 1.0
    return w * unit


def _quarters(lo, hi, n, g):
    """n multiples of 1/4 in [lo / 4, hi / 4]."""
    return torch.randint(lo, hi + 1, (n,), generator=g).float() / 4


def _ffn_exact_tail(D, F_, g, xvar, q2F):
    """W1, b1, W2, b2 of the exact class for an x of variance xvar: accumulator std 1.25, b1 = -1 + multiples of 1/4
    in [-1/2, 1/2] (about a fifth of the hidden units live), W2 with q2 = q2F / F (at most 0.19)."""
    W1 = sparse_w((F_, D), _EXACT_ACC_STD ** 2 / (D * xvar), g)
    b1 = -1 + _quarters(-2, 2, F_, g)
    W2 = sparse_w((D, F_), min(0.19, q2F / F_), g)
    return W1, b1, W2, _quarters(-4, 4, D, g)


FFN_KINDS_ = ('ffn', 'attn_out_ffn', 'pair', 'pair_ds')      # the entry points, in the planner's order


def _seed(case, cls):
    kind, D, F_, DB, M, debug = case[:6]
    return (FFN_KINDS_.index(kind) * 7 + debug) * 1000003 + D * 7919 + F_ * 131 + DB * 17 + M + (0 if cls == 'exact' else 5)


FFN_LN1_EPS_EXACT = 3.0


def ffn_direct_inputs(case, cls, dtype=None):
    return _ffn_direct_inputs(tuple(case[:7]), cls, dtype)


@functools.lru_cache(maxsize=3)
def _ffn_direct_inputs(case, cls, dtype):
    """The operands of a row of FFN_DIRECT_CASES as CPU f32 tensors.  cls 'exact' (dtype-independent: pass None) or
    'generic' (randn rounded to dtype, weights scaled by K^-1/2: generic_operands).

    Exact class, FFN: x multiples of 1/2 in [-1, 1]; W1, W2 in {0, +-1/2, +-1}, sparse; h comes out as multiples of
    1/4 and the output as multiples of 1/8 below 32: exact in bf16.
    Exact class, attention entry: A, Wo, bo dyadic, S = +-1 with D/2 of each sign per row, R = S - (A Wo^T + bo), so
    LayerNorm1's input is S whatever the summation order: mean 0, variance 1, and with eps1 = 3 rstd = 1/2; gamma1 in
    {1, 2}, beta1 in {+-1/4, +-3/4}: x = +-gamma1/2 + beta1 is a non-zero multiple of 1/4, far from any rounding tie
    (an inexact rsqrtf moves nothing: test_direct_refs_cpu.py).  h multiples of 1/8, the output of 1/16 below 16.
    Exact class, pairs: X, X0 multiples of 1/2, R of 1/4 in [-1, 1]; raw weights in {0, +-1/2, +-1} and scales in
    {1, 2}; b3 multiples of 1/4 in [0, 1]; Y multiples of 1/4, T of 1/8 below 32."""
    kind, D, F_, DB, M = case[:5]
    g = torch.Generator().manual_seed(_seed(case, cls))
    ex = cls == 'exact'
    d = {}
    if kind == 'ffn':
        if ex:
            d['x'] = exact_x((M, D), g)
            d['W1'], d['b1'], d['W2'], d['b2'] = _ffn_exact_tail(D, F_, g, 0.5, 30)
        else:
            d['x'], d['W1'] = generic_operands((M, D), (F_, D), D, dtype, g)
    elif kind == 'attn_out_ffn':
        if ex:
            d['A'] = exact_x((M, D), g)
            d['Wo'] = sparse_w((D, D), _EXACT_ACC_STD ** 2 / (D * 0.5), g)
            d['bo'] = _quarters(-4, 4, D, g)
            d['S'] = (torch.rand(M, D, generator=g).argsort(1) < D // 2).float() * 2 - 1
            d['R'] = (d['S'].double() - (d['A'].double() @ d['Wo'].double().T + d['bo'].double())).float()
            d['g1'] = torch.randint(1, 3, (D,), generator=g).float()
            d['be1'] = torch.tensor([-0.75, -0.25, 0.25, 0.75])[torch.randint(0, 4, (D,), generator=g)]
            d['eps1'] = FFN_LN1_EPS_EXACT
            # var(x) = E[gamma1^2] / 4 + E[beta1^2] = 5/8 + 5/16
            d['W1'], d['b1'], d['W2'], d['b2'] = _ffn_exact_tail(D, F_, g, 0.9375, 6)
        else:
            d['A'], d['Wo'] = generic_operands((M, D), (D, D), D, dtype, g)
            d['bo'] = torch.randn(D, generator=g)
            d['R'] = torch.randn(M, D, generator=g).to(dtype).float()
            d['g1'], d['be1'] = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
            d['eps1'] = 1e-5
            d['W1'] = (torch.randn(F_, D, generator=g) / D ** 0.5).to(dtype).float()
    if kind in ('ffn', 'attn_out_ffn'):
        if not ex:
            d['b1'] = torch.randn(F_, generator=g)
            d['W2'] = (torch.randn(D, F_, generator=g) / F_ ** 0.5).to(dtype).float()
            d['b2'] = torch.randn(D, generator=g)
        d['ln'] = (torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g), 1e-5)
        return d
    ds = kind == 'pair_ds'
    if ex:
        d['X'] = exact_x((M, D), g)
        qa = _EXACT_ACC_STD ** 2 / (D * 0.5 * 2.5) / (2 if ds else 1)     # E[s^2] = 5/2
        d['W3'], d['s3'] = sparse_w((F_, D), qa, g), torch.randint(1, 3, (F_,), generator=g).float()
        d['b3'] = _quarters(0, 4, F_, g)
        if ds:
            d['X0'] = exact_x((M, D), g)
            d['Wds'], d['sds'] = sparse_w((F_, D), qa, g), torch.randint(1, 3, (F_,), generator=g).float()
        else:
            d['R'] = torch.randint(-4, 5, (M, F_), generator=g).float() / 4
        d['W1'], d['s1'] = sparse_w((DB, F_), 2.0 / F_, g), torch.randint(1, 3, (DB,), generator=g).float()
        d['b1'] = _quarters(-4, 4, DB, g)
    else:
        d['X'] = torch.randn(M, D, generator=g).to(dtype).float()
        d['W3'], d['s3'] = torch.randn(F_, D, generator=g) / D ** 0.5, torch.rand(F_, generator=g) + 0.5
        d['b3'] = torch.randn(F_, generator=g)
        if ds:
            d['X0'] = torch.randn(M, D, generator=g).to(dtype).float()
            d['Wds'], d['sds'] = torch.randn(F_, D, generator=g) / D ** 0.5, torch.rand(F_, generator=g) + 0.5
        else:
            d['R'] = torch.randn(M, F_, generator=g).to(dtype).float()
        d['W1'], d['s1'] = torch.randn(DB, F_, generator=g) / F_ ** 0.5, torch.rand(DB, generator=g) + 0.5
        d['b1'] = torch.randn(DB, generator=g)
    return d


def ffn_direct_ref(case, d, dtype, ln=False, offset=0.0, drop=None, rows=None, dev='cpu'):
    """The reference of a row of FFN_DIRECT_CASES on its operands d (all rows, or the slice `rows`), on device `dev`.
    ln: the final LayerNorm on (FFN entries), with `offset` added to b2."""
    kind = case[0]

    def t(name, per_row=False):
        v = d[name][rows] if per_row and rows is not None else d[name]
        return v.to(dev)
    if kind in ('ffn', 'attn_out_ffn'):
        lnp = (d['ln'][0].to(dev), d['ln'][1].to(dev), d['ln'][2]) if ln else None
        b2 = t('b2') + offset
        if kind == 'ffn':
            return ffn_ref(t('x', True), t('W1'), t('b1'), t('W2'), b2, lnp, dtype, drop)
        return attn_out_ffn_ref(t('A', True), t('R', True), t('Wo'), t('bo'), (t('g1'), t('be1'), d['eps1']),
                                t('W1'), t('b1'), t('W2'), b2, lnp, dtype, drop)
    if kind == 'pair':
        return pair_ref(t('X', True), t('R', True), t('W3'), t('s3'), t('b3'), t('W1'), t('s1'), t('b1'), dtype, drop)
    return pair_ds_ref(t('X', True), t('X0', True), t('W3'), t('Wds'), t('s3'), t('sds'), t('b3'), t('W1'), t('s1'),
                       t('b1'), dtype, drop)


def ffn_direct_outputs(case, ref):
    """{name: f64 value before the output rounding} of what the entry point writes."""
    return {'y': ref['y']} if case[0] in ('ffn', 'attn_out_ffn') else {'Y': ref['preY'], 'T': ref['preT']}


def ffn_direct_gemms(case):
    """The weight matrices of a case's GEMMs, by their key in its operands (= the `drop` name of the references)."""
    return {'ffn': ('W1', 'W2'), 'attn_out_ffn': ('Wo', 'W1', 'W2'), 'pair': ('W3', 'W1'), 'pair_ds': ('W3', 'Wds', 'W1')}[case[0]]


def ffn_direct_generic_tol(case, d, ref, dtype, ln):
    """Per-element tolerance of each output of a generic-class row (derivation above ffn_generic_bound)."""
    kind, D, F_, DB = case[:4]
    r = OUT_ROUND[dtype]
    dev = ref['absA'].device
    if kind in ('pair', 'pair_ds'):
        K1 = 2 * D if kind == 'pair_ds' else D
        errA = 1.01 * (K1 + 64) * U32 * ref['absA'] + 4 * U32 * ref['majA']
        dY = (1 + r) * errA + 2 * r * ref['Y'].abs()
        W1a = ref['W1s'].abs()
        ET = dY @ W1a.T + 1.01 * (F_ + 64) * U32 * ((ref['Y'].abs() + dY) @ W1a.T) + 4 * U32 * ref['majB']
        return {'Y': out_round_bound(errA, ref['preY'], dtype), 'T': out_round_bound(ET, ref['preT'], dtype)}
    W1a, W2a = d['W1'].double().abs().to(dev), d['W2'].double().abs().to(dev)
    dxA = dx = None
    if kind == 'attn_out_ffn':
        # x: the out-projection's sums (as phase A, the residual among the additions) through LayerNorm1, the f32
        # LayerNorm's own error (ln_epilogue_ref: y_c u yA), then the two roundings of x as for the hidden
        E1 = 1.01 * (D + 64) * U32 * ref['absO'] + 4 * U32 * ref['majO']
        l1 = ref['ln1']
        ex = ln_propagate(E1, ref['pre1'], d['g1'].to(dev), d['eps1']) + l1['y_c'] * U32 * l1['yA']
        dx = (1 + r) * ex + 2 * r * ref['x'].abs()
        dxA = dx @ W1a.T
    E, _ = ffn_generic_bound(ref['absA'], ref['majA'], ref['h'], W2a, ref['majB'], D, F_, dtype, dxA, dx)
    if not ln:
        return {'y': out_round_bound(E, ref['pre'], dtype)}
    _, tol = ffn_ln_tol(ref['pre'], d['ln'], dtype)
    return {'y': ln_propagate(E, ref['pre'], d['ln'][0].to(dev), d['ln'][2]) + tol.to(dev)}


# ------------------------------------------------------- attention forward, kernel by kernel
# Cases, expected values and the bound of tests/test_attn_direct_gpu.py (csrc/attn.hip: mha_resident_kernel,
# mha_stream_kernel; csrc/ops.hip: mha_kernel).  Every case has ATTN_B batches with different masks and ATTN_HEADS
# heads (odd head offsets: at head_dim 36 an odd head starts 8-byte, not 16-byte aligned); codes, values and the
# query -> key assignment differ per batch, head and query.
ATTN_KT = 128                       # keys per tile of the streaming kernel (kernels.MHA_STREAM_KT)
ATTN_RESIDENT_MAXK = {32: 384, 36: 640}
ATTN_B, ATTN_HEADS = 2, 3
ATTN_U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoffs
ATTN_INST = ([(kern, dt, D) for kern in ('resident', 'stream') for dt in (torch.bfloat16, torch.float16) for D in (32, 36)]
             + [('fma', dt, D) for dt in (torch.float32, torch.bfloat16, torch.float16) for D in (16, 32, 36, 64)])
# (Lq, Lk): every Lk of {1, 31, 32, 33, 37, KT - 1, KT, KT + 1, 2 KT + 5, 3 KT} and every Lq of {1, 15, 16, 17, 63, 64,
# 65, 129}; the two three-tile cases have enough queries to select every slot of a block in each tile
ATTN_SHAPES = [(1, 1), (15, 31), (16, 32), (17, 33), (63, 37), (64, ATTN_KT - 1), (65, ATTN_KT), (129, ATTN_KT + 1),
               (129, 2 * ATTN_KT + 5), (129, 3 * ATTN_KT)]
ATTN_FMA_SHAPES = [(17, 63), (64, 64), (65, 65), (129, 129)]        # the FMA kernel's 64-key tile
ATTN_MAIN = (129, 2 * ATTN_KT + 5)


def attn_shapes(kernel, D):
    """The (Lq, Lk) of one instantiation: the common list, the FMA kernel's tile edges, the resident caps (cap - 31,
    cap) and, as 'stream', cap + 1 -- which the default knob sends there."""
    s = list(ATTN_SHAPES)
    if kernel == 'fma':
        s += ATTN_FMA_SHAPES
    if kernel == 'resident':
        s += [(16, ATTN_RESIDENT_MAXK[D] - 31), (65, ATTN_RESIDENT_MAXK[D])]
    if kernel == 'stream':
        s += [(65, ATTN_RESIDENT_MAXK[D] + 1)]
    return s


def _attn_split(t, heads):
    B, L, E = t.shape
    return t.view(B, L, heads, E // heads).transpose(1, 2)


def _attn_merge(t):
    B, H, L, D = t.shape
    return t.transpose(1, 2).reshape(B, L, H * D)


def attn_bits(t):
    """The bit patterns of t as integers (exact comparisons: NaN-free, +0 != -0)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


_ATTN_FMT = {torch.float32: (torch.int32, 8, 23, 227), torch.bfloat16: (torch.int16, 8, 7, 227),
             torch.float16: (torch.int16, 5, 10, 30)}


def attn_random_values(shape, dtype, g):
    """Arbitrary finite bit patterns of dtype, subnormals included: sign, exponent field 0 .. emax, mantissa, each
    uniform.  bf16 / f32 stay below 2^101, so that no f32 partial sum of the kernels can overflow (a partial O^T
    holds p v of keys that a later rescale by exactly 0 removes: inf * 0 would be NaN in any online softmax); -0 is
    left out (x + -0 = +0 in the accumulator)."""
    it, eb, mb, emax = _ATTN_FMT[dtype]
    sign = torch.randint(0, 2, shape, generator=g)
    ex = torch.randint(0, emax + 1, shape, generator=g)
    mant = torch.randint(0, 2 ** mb, shape, generator=g)
    bits = (sign << (eb + mb)) | (ex << mb) | mant
    bits = torch.where((ex == 0) & (mant == 0), torch.zeros_like(bits), bits)
    width = 32 if it == torch.int32 else 16
    bits = torch.where(bits >= 2 ** (width - 1), bits - 2 ** width, bits)
    return bits.to(it).view(dtype)


def attn_special_rows(D, dtype):
    """(4, D): zeros; negatives; the largest finite value with alternating sign; subnormals (the smallest and the
    largest, alternating sign)."""
    fi = torch.finfo(dtype)
    alt = torch.tensor([1.0, -1.0]).repeat(D)[:D].double()
    neg = -(torch.arange(D).double() % 7 + 1) * 0.375
    big = alt * fi.max
    tiny = fi.smallest_normal * 2.0 ** -{torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}[dtype]
    sub = torch.where(torch.arange(D) % 4 < 2, torch.tensor(tiny, dtype=torch.float64),
                      torch.tensor(fi.smallest_normal - tiny, dtype=torch.float64)) * alt
    rows = torch.stack([torch.zeros(D, dtype=torch.float64), neg, big, sub]).to(dtype)
    assert torch.equal(rows.double(), torch.stack([torch.zeros(D, dtype=torch.float64), neg, big, sub]))
    return rows


def _attn_codes(n, D, g):
    """n distinct +-1 codewords of length D, (n, D) int64."""
    low = torch.randperm(2 ** 16, generator=g)[:n]
    bits = [(low >> d) & 1 for d in range(min(D, 16))] + [torch.randint(0, 2, (n,), generator=g) for _ in range(D - 16)]
    return torch.stack(bits, 1) * 2 - 1


def attn_pair_keys(D, Lk, kt=ATTN_KT):
    """Key indices (lo[d], hi[d]) of the pair that differs in head dim d only, d < min(D, Lk // 2): lo in the first
    blocks, hi from the last block of the second tile where that fits (so one of the pair sits blocks, and a tile,
    before the other), and the 'middle' block index (None below three blocks)."""
    npair = min(D, Lk // 2)
    nblk = (Lk + 31) // 32
    mid = min(2 * kt // 32 - 1, nblk - 2) if nblk >= 3 else None
    lo = list(range(npair))
    if mid is not None and mid * 32 >= npair and mid * 32 + npair <= Lk:
        hi = list(range(mid * 32, mid * 32 + npair))
    else:
        hi = list(range(npair, 2 * npair))
    return lo, hi, mid


def _attn_priority(D, Lk, kt):
    lo, hi, mid = attn_pair_keys(D, Lk, kt)
    nblk = (Lk + 31) // 32
    order = lo + hi + list(range(min(32, Lk)))
    if mid is not None:
        order += list(range(mid * 32, mid * 32 + 32))
    order += list(range((nblk - 1) * 32, Lk)) + list(range(Lk))
    return list(dict.fromkeys(order))


def _attn_select_mask(D, Lk, mode, kt):
    """The key masks of a selection case (B, Lk).  'pairs': in batch b the pair member a_d (lo[d] for even d, hi[d]
    for odd d) of every d = b mod 3 -- its query then selects the other member, the nearest live key -- and every
    7th key outside the pairs.  'edges': batch 0 masks the first block, a middle block and the last (ragged) block,
    batch 1 the whole first tile (the first block below two tiles).  'last': batch 0 keeps key Lk - 1 only, batch 1
    nothing."""
    mask = torch.zeros(ATTN_B, Lk, dtype=torch.bool)
    lo, hi, _ = attn_pair_keys(D, Lk, kt)
    nblk = (Lk + 31) // 32
    if mode == 'pairs':
        paired = set(lo + hi)
        for b in range(ATTN_B):
            for d in range(len(lo)):
                if d % 3 == b:
                    mask[b, lo[d] if d % 2 == 0 else hi[d]] = True
            for j in range(3 + b, Lk, 7):
                if j not in paired:
                    mask[b, j] = True
    elif mode == 'edges':
        mask[0, :32] = True
        mask[0, (nblk // 2) * 32:(nblk // 2) * 32 + 32] = True
        mask[0, (nblk - 1) * 32:] = True
        mask[1, :kt if Lk > kt else 32] = True
    elif mode == 'last':
        mask[0, :Lk - 1] = True
        mask[1] = True
    return mask


def _attn_select_try(D, Lq, Lk, dtype, mode, kt, seed):
    B, H = ATTN_B, ATTN_HEADS
    g = torch.Generator().manual_seed(77003 * seed + 131 * D + 17 * Lq + Lk + {'pairs': 0, 'edges': 1, 'last': 2}[mode] * 7919)
    lo, hi, mid = attn_pair_keys(D, Lk, kt)
    codes = torch.stack([torch.stack([_attn_codes(Lk, D, g) for _ in range(H)]) for _ in range(B)])   # (B, H, Lk, D)
    for d in range(len(lo)):
        codes[:, :, hi[d]] = codes[:, :, lo[d]]
        codes[:, :, hi[d], d] *= -1
    mask = _attn_select_mask(D, Lk, mode, kt)
    prio = _attn_priority(D, Lk, kt)
    target = torch.zeros(B, H, Lq, dtype=torch.long)
    for b in range(B):
        # a masked pair member stays a target: its query selects the other member
        live = [j for j in prio if not mask[b, j] or (mode == 'pairs' and j in set(lo + hi))]
        tl = live if live else prio
        for h in range(H):
            perm = torch.randperm(Lq, generator=g)
            target[b, h] = torch.tensor([tl[int(i) % len(tl)] for i in perm])
    qcode = torch.gather(codes, 2, target[..., None].expand(B, H, Lq, D))
    S = 64 * (qcode @ codes.transpose(-1, -2))                                         # exact integers
    Sm = S.masked_fill(mask[:, None, None, :], -2 ** 40)
    top = Sm.topk(min(2, Lk), -1).values
    alive = ~mask.all(1)
    if Lk > 1 and (top[alive][..., 0] - top[alive][..., 1]).min() < 128:
        return None
    sel = Sm.argmax(-1)                                                                 # (B, H, Lq)
    v = attn_random_values((B, H, Lk, D), dtype, g)
    special = attn_special_rows(D, dtype)
    for i in range(min(4, Lk)):
        v[:, :, prio[i]] = special[i]
    huge = special[2]
    v = torch.where(mask[:, None, :, None], huge.expand(B, H, Lk, D), v)
    expected = torch.gather(v, 2, sel[..., None].expand(B, H, Lq, D))
    expected = torch.where(alive[:, None, None, None], expected, torch.zeros_like(expected))
    return {'q': _attn_merge(64 * qcode).to(dtype), 'k': _attn_merge(codes).to(dtype), 'v': _attn_merge(v), 'mask': mask,
            'scale': 1.0, 'sel': sel, 'target': target, 'expected': _attn_merge(expected), 'codes': codes, 'scores': S,
            'heads': H, 'mode': mode}


@functools.lru_cache(maxsize=None)
def attn_select_case(D, Lq, Lk, dtype, mode='pairs', kt=ATTN_KT):
    """Class 1.  Keys are distinct +-1 codewords, query i is 64 code(target(i)), scale = 1: every score is an integer
    multiple of 128 apart from every other (64 (D - 2 hamming)), exact in f32, so the softmax is exactly one-hot
    on the best live key `sel` and the output row is v[sel] bit for bit.  The builder re-seeds until the best live
    key of every query leads by >= 128 (the masked-best-match queries need a unique nearest live key)."""
    for seed in range(32):
        case = _attn_select_try(D, Lq, Lk, dtype, mode, kt, seed)
        if case is not None:
            return case
    raise AssertionError('attn_select_case: no seed gives a score gap of 128')


def attn_tie_groups(kt=ATTN_KT):
    """Class 2's tied key sets at Lk = 2 kt + 5, name -> key indices (disjoint)."""
    b3, b7 = kt - 32, 2 * kt - 32           # the last blocks of tiles 0 and 1
    groups = {
        'lane8': [4, 5, 6, 7, 20, 21, 22, 23],                  # the eight keys of lane group 1 of block 0
        'lane4': [8, 9, 10, 11],
        'lane2': [12, 28],
        'groups4': [b3, b3 + 4, b3 + 8, b3 + 12],                # one key of each lane group: the two cross-lane sums
        'groups16': list(range(b7, b7 + 16)),
        'block32': list(range(kt + 64, kt + 96)),
        'consec64': list(range(32, 96)),                         # two whole consecutive blocks: alpha = 1 between them
        'consec2': [kt + 5, kt + 37],
        'edge4': [kt - 2, kt - 1, kt, kt + 1],                   # across the edge of tiles 0 and 1
        'tiles02_2': [3, 2 * kt + 3],                            # tiles 0 and 2: the same buffer, reused
        'tiles02_8': [1, 2, 13, 14, 2 * kt, 2 * kt + 1, 2 * kt + 2, 2 * kt + 4],
    }
    flat = [j for ks in groups.values() for j in ks]
    assert len(flat) == len(set(flat)) and max(flat) < 2 * kt + 5
    return groups


ATTN_TIE_DECOY = (15, 'lane2')              # a masked key that carries a group's codeword and huge values


@functools.lru_cache(maxsize=None)
def attn_tie_case(D, Lq, dtype, kt=ATTN_KT):
    """Class 2.  As class 1, but the n in {2, .., 64} keys of a group share the selected codeword: p is 1 on n keys, l
    is n, the output is the mean of their values -- nonzero multiples of 1/4 up to 3/4, so the f32 sums are exact,
    the mean (an integer of at most 8 bits over 4 n) is representable in bf16 / f16 and survives the final rounding."""
    B, H, Lk = ATTN_B, ATTN_HEADS, 2 * kt + 5
    groups = attn_tie_groups(kt)
    names = sorted(groups)
    for seed in range(32):
        g = torch.Generator().manual_seed(90001 * seed + 131 * D + Lq)
        codes = torch.stack([torch.stack([_attn_codes(Lk, D, g) for _ in range(H)]) for _ in range(B)])
        for ks in groups.values():
            codes[:, :, ks] = codes[:, :, ks[:1]]
        mask = torch.zeros(B, Lk, dtype=torch.bool)
        codes[:, :, ATTN_TIE_DECOY[0]] = codes[:, :, groups[ATTN_TIE_DECOY[1]][0]]
        mask[:, ATTN_TIE_DECOY[0]] = True
        grouped = {j for ks in groups.values() for j in ks}
        for b in range(B):
            for j in range(30 + b, Lk, 9):
                if j not in grouped:
                    mask[b, j] = True
        gi = torch.stack([torch.stack([torch.randperm(Lq, generator=g) % len(names) for _ in range(H)]) for _ in range(B)])
        first = torch.tensor([groups[n][0] for n in names])[gi]
        qcode = torch.gather(codes, 2, first[..., None].expand(B, H, Lq, D))
        S = 64 * (qcode @ codes.transpose(-1, -2))
        Sm = S.masked_fill(mask[:, None, None, :], -2 ** 40)
        best = Sm.amax(-1, keepdim=True)
        tied = Sm == best
        size = torch.tensor([len(groups[n]) for n in names])[gi]
        rest = Sm.masked_fill(tied, -2 ** 40).amax(-1, keepdim=True)
        if not torch.equal(tied.sum(-1), size) or (best - rest).min() < 128:
            continue
        v = attn_random_values((B, H, Lk, D), dtype, g)
        m4 = (torch.randint(1, 4, (B, H, Lk, D), generator=g) * (torch.randint(0, 2, (B, H, Lk, D), generator=g) * 2 - 1)) / 4.0
        gmask = torch.zeros(Lk, dtype=torch.bool)
        gmask[sorted(grouped)] = True
        v = torch.where(gmask[None, None, :, None], m4.to(dtype), v)
        v = torch.where(mask[:, None, :, None], attn_special_rows(D, dtype)[2].expand(B, H, Lk, D), v)
        mean = (tied.double() @ v.double()) / size[..., None].double()
        expected = mean.to(dtype)
        assert torch.equal(expected.double(), mean), 'attn_tie_case: a mean is not representable'
        return {'q': _attn_merge(64 * qcode).to(dtype), 'k': _attn_merge(codes).to(dtype), 'v': _attn_merge(v),
                'mask': mask, 'scale': 1.0, 'group': gi, 'names': names, 'tied': tied, 'expected': _attn_merge(expected),
                'mean64': _attn_merge(mean), 'scores': S, 'heads': H}
    raise AssertionError('attn_tie_case: no seed gives a score gap of 128')


ATTN_VARIANTS = ('plain', 'wide', 'offset')
ATTN_MASKS = ('random', 'none', 'allfalse', 'first_block', 'first_tile', 'middle_block', 'last_block', 'last_only',
              'dead_batch')


def attn_generic_mask(Lk, mode, g, kt=ATTN_KT):
    if mode == 'none':
        return None
    mask = torch.zeros(ATTN_B, Lk, dtype=torch.bool)
    nblk = (Lk + 31) // 32
    if mode == 'random':
        mask = torch.rand(ATTN_B, Lk, generator=g) < 0.2
        mask[0, 0] = False
        mask[1, Lk - 1] = False
    elif mode == 'first_block':                  # m stays -inf through the first block (batch 1: the first two)
        mask[0, :32] = True
        mask[1, :64] = True
    elif mode == 'first_tile':
        mask[:, :kt] = True
        mask[1, kt:kt + 7] = True
    elif mode == 'middle_block':
        mask[0, (nblk // 2) * 32:(nblk // 2) * 32 + 32] = True
        mask[1, 32:64] = True
    elif mode == 'last_block':
        mask[0, (nblk - 1) * 32:] = True
        mask[1, (nblk - 2) * 32:] = True
    elif mode == 'last_only':
        mask[:, :Lk - 1] = True
    elif mode == 'dead_batch':
        mask[1] = True
        mask[0, 5] = True
    return mask


@functools.lru_cache(maxsize=None)
def attn_generic_case(D, Lq, Lk, dtype, variant='plain', maskmode='random'):
    """Class 3: N(0, 1) operands rounded to dtype, scale D^-0.5.  'wide': q times 15, so scores reach +-60; 'offset':
    dim 0 of every key is 4 and dim 0 of every query 50 sqrt(D), a common score offset of 200 that the softmax
    cancels and the f32 score arithmetic does not.  With the f64 reference of the rounded operands, the bound's
    ingredients and torch's CPU f32 SDPA."""
    H = ATTN_HEADS
    q, k, v, _ = attn_case(ATTN_B, H, D, Lq, Lk, seed=5 + ATTN_VARIANTS.index(variant), qscale=15.0 if variant == 'wide' else 1.0)
    q, k, v = q.clone(), k.clone(), v.clone()
    if variant == 'offset':
        k[..., ::D] = 4.0
        q[..., ::D] = 50.0 * math.sqrt(D)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    g = torch.Generator().manual_seed(D * 31 + Lk + ATTN_MASKS.index(maskmode) * 1009)
    mask = attn_generic_mask(Lk, maskmode, g)
    scale = D ** -0.5
    ref = attn_ref(q, k, v, torch.zeros_like(q), H, scale, key_mask=mask)
    case = {'q': q, 'k': k, 'v': v, 'mask': mask, 'scale': scale, 'heads': H, 'o': ref['o'], 'oA': ref['oA']}
    case['sdpa'] = attn_sdpa_f32(q, k, v, H, scale, mask)
    return case


def attn_sdpa_f32(q, k, v, heads, scale, mask):
    """torch's CPU f32 scaled_dot_product_attention on the same (rounded) operands, 0 on a batch without a live key:
    the yardstick."""
    m = None
    dead = torch.zeros(q.shape[0], dtype=torch.bool)
    if mask is not None:
        dead = mask.all(1)
        m = mask.clone()
        m[dead] = False
        m = ~m[:, None, None, :]
    o = F.scaled_dot_product_attention(_attn_split(q.float(), heads), _attn_split(k.float(), heads),
                                       _attn_split(v.float(), heads), attn_mask=m, scale=scale)
    o = _attn_merge(o).double()
    o[dead] = 0
    return o


def attn_fwd_bound(case, kernel, dtype):
    """Per-element bound on |kernel output - f64 attention| of a class-3 case, from the kernels' arithmetic; u = 2^-24
    (f32), u16 the unit roundoff of the 16-bit type (2^-8 bf16, 2^-11 f16).  The kernels compute, key block by key
    block (32 keys: attn_block; one key: the FMA kernel), s = scale q.k (+ 0 / -inf key bias), the running max m,
    p = __expf(s - m), l = l alpha + sum p, O = O alpha + p v with alpha = __expf(m_old - m_new), and at the end
    O / l rounded to the output type.  With P the exact softmax, o = P V, oA = P |V| (attn_ref):

    (a) output rounding: u_out |o|, plus half the subnormal spacing of the output type (2^-25 in f16).
    (b) MFMA kernels only: p is rounded to the 16-bit type as the B operand of O^T += V^T P^T while l sums the
        unrounded p: relative u16 on every normal p -- u16 oA -- and an absolute part for p below the smallest
        normal.  Facts this rests on: Cvt<f16_t>::from is a plain float -> _Float16 cast (v_cvt_f16_f32, round to
        nearest even; the kernels are built with hipcc's default mode, which keeps f16 and f32 subnormals), and
        the MFMA never flushes its C / D and is modelled as taking the f16 subnormal operand as it is: the
        absolute error is half the subnormal spacing, 2^-25 per live key, scaled by 1 / l (l >= 1 in units of the
        largest p).  f32_to_bf16 is a plain __bf16 cast (v_cvt_pk_bf16_f32: round to nearest even, NaN kept);
        bf16 shares f32's exponent range, so a p below 2^-126 is already an f32 subnormal: 2^-126 per live key
        covers either treatment.  The 257-key case of attn_subnormal_case tells 'kept' from 'flushed' in f16:
        flushed, the output misses by 2^-8.
    (c) score error.  The products of two 16-bit values are exact in f32; S^T accumulates n = 32 KSTEPS of them
        (64 at head_dim 36: the padded length), each addition committing at most one ulp (2 u, which covers
        truncation as well as round to nearest), then one rounding of the scale multiply; the key bias adds 0 or
        -inf exactly.  The FMA kernel rounds q scale once, then runs D / 4 fma and two shuffle additions: n = D / 4
        + 2.  ds = (2 n + 2) u scale sum_d |q_d k_d| per (query, key); an error of the running max itself is common
        to numerator and denominator and cancels.
    (d) __expf(x) = exp2(x log2 e): the rounding of s - m and of the argument, 2 |x| u, and 4 u for the result's
        ulps.  Over a key's own exp and the later rescales, the arguments add up to exactly m_final - s, so
        a key's weight has the relative error e = ds + 2 (m - s) u + 4 u (steps + 1), steps = ceil(Lk / 32) (FMA:
        ceil(Lk / 4) keys per wave + the merge).
        (c) and (d) enter numerator and denominator: sum_j P_j (|v_j| + |o|) e_j, which is at most 2 max(e) oA.
    (e) f32 accumulation of l and O^T: a multiply and an add per step, and the 32-term sum of an MFMA:
        2 (2 steps + 32) u oA, and 3 u |o| for 1 / l and the final product.
    Elements with oA = 0 (no live key, or only zero values) must be exactly 0."""
    q, k, v, mask, scale, H = (case[n] for n in ('q', 'k', 'v', 'mask', 'scale', 'heads'))
    D = q.shape[-1] // H
    Lk = k.shape[1]
    u = U32
    Q, K_, V = _attn_split(q.double(), H), _attn_split(k.double(), H), _attn_split(v.double(), H)
    S = Q @ K_.transpose(-1, -2) * scale
    SA = Q.abs() @ K_.abs().transpose(-1, -2) * scale
    live = torch.ones(q.shape[0], Lk, dtype=torch.bool) if mask is None else ~mask
    S = S.masked_fill(~live[:, None, None, :], float('-inf'))
    mx = S.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = (S - mx).exp()
    den = e.sum(-1, keepdim=True)
    P = e / torch.where(den > 0, den, torch.ones_like(den))
    mfma = kernel != 'fma'
    n = 32 * (2 if D == 36 else 1) if mfma else D // 4 + 2
    steps = (Lk + 31) // 32 if mfma else (Lk + 3) // 4 + 1
    X = torch.where(P > 0, mx - S, torch.zeros_like(S))
    ej = (2 * n + 2) * u * SA + 2 * X * u + 4 * u * (steps + 1)
    Pe = P * ej
    o, oA = _attn_split(case['o'], H), _attn_split(case['oA'], H)
    bound = Pe @ V.abs() + o.abs() * Pe.sum(-1, keepdim=True)
    bound = bound + 2 * (2 * steps + 32) * u * oA + 3 * u * o.abs()
    tiny = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}[dtype]
    bound = bound + ATTN_U[dtype] * o.abs() + tiny
    if mfma:
        sub = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25}[dtype]
        absV = (live[:, None, :, None].double() * V.abs()).sum(2, keepdim=True)
        bound = bound + ATTN_U[dtype] * oA + sub * absV / torch.where(den > 0, den, torch.ones_like(den))
    return _attn_merge(torch.where(oA > 0, bound, torch.zeros_like(bound)))


def attn_ratio(got64, case, bound):
    """(worst |got - o| / bound over the elements with oA > 0, their share of all elements, whether every other
    element is exactly 0)."""
    cmp = case['oA'] > 0
    err = (got64 - case['o']).abs()
    worst = (err[cmp] / bound[cmp]).max().item() if cmp.any() else 0.0
    return worst, cmp.double().mean().item(), bool((got64[~cmp] == 0).all())


@functools.lru_cache(maxsize=None)
def attn_subnormal_case(D, dtype):
    """One key at p = 1 and 256 keys near p = 2^-16 (scale 1, q = e_0, the keys' dim 0 is 0 and -11.09), every value 1:
    the exact output is 1.  In f16 those p are subnormal operands of P V: kept (spacing 2^-24), the kernel's sum
    misses 1 by at most 256 2^-25; flushed, it gives 1 / (1 + 2^-8)."""
    B, H, Lq, Lk = ATTN_B, ATTN_HEADS, 17, 257
    E = H * D
    q, k = torch.zeros(B, Lq, E), torch.zeros(B, Lk, E)
    q[..., ::D] = 1.0
    k[:, 1:, ::D] = -16 * math.log(2.0)
    v = torch.ones(B, Lk, E)
    return _attn_make(q.to(dtype), k.to(dtype), v.to(dtype), H, 1.0)


def _attn_bias_parts(D, dtype, nAs, Lq=1, Lk=257):
    """One batch of the bias case: head h has key 0 at score 0 (p = 1, value 0), nAs[h] keys of value 1 whose p sits
    just below a rounding midpoint of the 16-bit type at 1/2 (rounded down by almost u16 relative) and value-0 keys
    whose p sits just above it (rounded up).  scale 1; q = e_0 + 2^-10 e_1, so a key's score is k_0 + 2^-10 k_1: a
    16-bit k_0 and its 16-bit residual place the score within 2^-18 of its target, the midpoint being 2^-13 (bf16) /
    2^-16 (f16) away in relative terms."""
    t = {torch.bfloat16: 8, torch.float16: 11}[dtype]
    H = len(nAs)
    xs = {'A': math.log((1 + 2.0 ** -t - 2.0 ** -(t + 5)) / 2), 'B': math.log((1 + 2.0 ** -t + 2.0 ** -(t + 5)) / 2)}
    q, k, v = torch.zeros(1, Lq, H, D), torch.zeros(1, Lk, H, D), torch.zeros(1, Lk, H, D)
    q[..., 0], q[..., 1] = 1.0, 2.0 ** -10
    for h, nA in enumerate(nAs):
        for j in range(1, Lk):
            x = xs['A' if j <= nA else 'B']
            k0 = torch.tensor(x).to(dtype).double().item()
            k[0, j, h, 0], k[0, j, h, 1] = k0, (x - k0) * 2.0 ** 10
        v[0, 1:nA + 1, h] = 1.0
    return q.reshape(1, Lq, H * D).to(dtype), k.reshape(1, Lk, H * D).to(dtype), v.reshape(1, Lk, H * D).to(dtype)


def _attn_make(q, k, v, H, scale, mask=None):
    ref = attn_ref(q, k, v, torch.zeros_like(q), H, scale, key_mask=mask)
    return {'q': q, 'k': k, 'v': v, 'mask': mask, 'scale': scale, 'heads': H, 'o': ref['o'], 'oA': ref['oA'],
            'sdpa': attn_sdpa_f32(q, k, v, H, scale, mask)}


@functools.lru_cache(maxsize=None)
def attn_bias_case(D, dtype):
    """The class-3 case built for the one systematic term of the bound, (b): with l summed from the unrounded p, the
    kernels' output is low by almost u16 oA -- inside the bound.  A kernel that summed l from the rounded p would
    be low by almost 2 u16 oA here (the value-0 keys inflate its l), and over the bound wherever the output rounding
    goes the same way: the counts of value-1 keys per head are the first six, from 1 up, at which the f64 model of
    that kernel is over the bound (test_direct_refs_cpu.py runs the mutation on this case)."""
    good = []
    for nA in range(1, 200):
        c = _attn_make(*_attn_bias_parts(D, dtype, [nA]), 1, 1.0)
        bound = attn_fwd_bound(c, 'resident', dtype)
        r = [attn_ratio(attn_blockwise(c, m, True, pround=dtype).to(dtype).double(), c, bound)[0] for m in (None, 'l_rounded')]
        if r[0] < 1.0 < r[1]:
            good.append(nA)
        if len(good) == ATTN_B * ATTN_HEADS:
            break
    assert len(good) == ATTN_B * ATTN_HEADS, good
    parts = [_attn_bias_parts(D, dtype, good[b * ATTN_HEADS:(b + 1) * ATTN_HEADS], Lq=17) for b in range(ATTN_B)]
    return _attn_make(*(torch.cat(t) for t in zip(*parts)), ATTN_HEADS, 1.0)


ATTN_MUTATIONS = ('swap', 'drop_dim35', 'drop_dim0', 'mask_shift', 'skip_rescale', 'drop_block', 'l_rounded')


def attn_blockwise(case, mut=None, arg=None, pround=None, kt=ATTN_KT):
    """The kernels' block step restated in f64: 32-key blocks in order, running max m, l = l alpha + sum p,
    O = O alpha + p V, O / l at the end (0 without a live key); exp(x) is 0 below -104, as in f32.  pround: a 16-bit
    type p is rounded to for P V (l keeps the unrounded p) -- the model of the MFMA kernels.  mut, one of
    ATTN_MUTATIONS, breaks it the way a kernel could be broken:
      'swap' (j1, j2): two keys of one block swapped against their values;
      'drop_dim35' / 'drop_dim0': that head dim lost from q.k;
      'mask_shift' (b, j): the mask byte of key j of batch b applied to key j + 1;
      'skip_rescale' i: block i does not rescale O (l is rescaled);
      'drop_block' i: block i contributes nothing (a tile's last block, lost at the buffer swap);
      'l_rounded': l sums the rounded p."""
    q, k, v, mask, scale, H = (case[n] for n in ('q', 'k', 'v', 'mask', 'scale', 'heads'))
    B, Lk = k.shape[0], k.shape[1]
    Q, K_, V = _attn_split(q.double(), H).clone(), _attn_split(k.double(), H), _attn_split(v.double(), H).clone()
    km = torch.zeros(B, Lk, dtype=torch.bool) if mask is None else mask.clone()
    if mut == 'swap':
        V[:, :, list(arg)] = V[:, :, list(arg)[::-1]]
    elif mut in ('drop_dim35', 'drop_dim0'):
        Q[..., int(mut[8:])] = 0
    elif mut == 'mask_shift':
        km[arg[0], arg[1]], km[arg[0], arg[1] + 1] = False, True
    S = (Q @ K_.transpose(-1, -2) * scale).masked_fill(km[:, None, None, :], float('-inf'))
    ninf = float('-inf')

    def ex(x):
        return torch.where(x < -104.0, torch.zeros_like(x), x.exp())
    m = torch.full(S.shape[:-1] + (1,), ninf, dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros_like(Q)
    for i, k0 in enumerate(range(0, Lk, 32)):
        if mut == 'drop_block' and i == arg:
            continue
        s = S[..., k0:k0 + 32]
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        dead = mn == ninf
        safe = torch.where(dead, torch.zeros_like(mn), mn)
        alpha = torch.where(dead | (m == ninf), torch.where(dead, torch.ones_like(m), torch.zeros_like(m)), ex(m - safe))
        p = torch.where(dead, torch.zeros_like(s), ex(s - safe))
        pr = p if pround is None else p.to(pround).double()
        l = l * alpha + (pr if mut == 'l_rounded' else p).sum(-1, keepdim=True)
        o = o * (torch.ones_like(alpha) if mut == 'skip_rescale' and i == arg else alpha) + pr @ V[:, :, k0:k0 + 32]
        m = mn
    return _attn_merge(torch.where(l > 0, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o)))


def attn_mutation_arg(mut, case, kt=ATTN_KT):
    """Where a mutation strikes in a case (None: it cannot strike there): the swap and the shifted mask byte in the
    last block of the second tile, the skipped rescale there too, the dropped block the last block of the first tile."""
    Lk = case['k'].shape[1]
    D = case['q'].shape[-1] // case['heads']
    j = 2 * kt - 32
    if mut == 'swap':           # (in a tie case: the last key of 'groups16' and its neighbour outside the group)
        return (j + 15, j + 16) if j + 16 < Lk else ((0, 1) if Lk > 1 else None)
    if mut == 'drop_dim35':
        return True if D > 35 else None
    if mut == 'drop_dim0':
        return True
    if mut == 'mask_shift':
        if case['mask'] is None:
            return None
        if 'tied' in case:      # the decoy's byte moves on: the decoy joins its group's tie
            return (0, ATTN_TIE_DECOY[0])
        for b in range(case['mask'].shape[0]):
            for jj in list(range(min(j, Lk - 1), Lk - 1)) + list(range(0, min(j, Lk - 1))):
                if case['mask'][b, jj] and not case['mask'][b, jj + 1]:
                    return (b, jj)
        return None
    if mut == 'skip_rescale':
        return j // 32 if j < Lk else None
    if mut == 'drop_block':
        return kt // 32 - 1 if kt < Lk else None
    return True


# ======================= the stem (csrc/stem.hip) and the direct 3x3 (csrc/conv3x3.hip), path by path
# The case tables and references of tests/test_stem_conv3x3_direct_gpu.py.  The two operand classes are
# gemm.hip's (above): EXACT -- the image / activation from exact_x, the weights from exact_w at the
# filter's K, scale and bias from exact_epilogue: every f32 partial sum is exact in any order and the
# kernel must equal the f64 result rounded once; GENERIC -- randn operands under gemm_generic_bound.
#   'c3':   x (B, H, W, 64) NHWC, w (64, 64, 3, 3) OIHW, stride 1, pad 1, K = 576
#   'stem': x (B, 3, H, W) f32 NCHW image, w (64, 3, 7, 7) OIHW, stride 2, pad 3, K = 147
FRONT_GEO = {'c3': (3, 1, 1, 64, 576), 'stem': (7, 2, 3, 3, 147)}       # filter, stride, pad, Cin, K
FRONT_FAULTS = ('drop_tap', 'left_halo', 'prev_image_row', 'swap_kw_c')


def conv_taps64(x_nhwc, w_ohwi, stride, pad, fault=None):
    """The convolution as a plain f64 sum over the filter taps of (shifted, strided input slice) @
    (the tap's (Cin, Cout) weights) -> (B*Ho*Wo, Cout), on the operands' device.  No im2col and no
    library convolution: it runs wherever an f64 matmul does, and a fault is one line:
      drop_tap        one (kh, kw, c) weight (the last row's middle tap, last channel) is left out;
      left_halo       the padding columns left of the image repeat column 0 instead of zeros;
      prev_image_row  the padding row just above image b holds the last row of image b - 1;
      swap_kw_c       the weights of (kw, c) = (0, 0) and (KW - 1, Cin - 1) of the middle row trade places."""
    x, w = x_nhwc.double(), w_ohwi.double()
    B, H, W, C = x.shape
    Co, KH, KW, _ = w.shape
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    Ho, Wo = out_size(H, W, KH, KW, stride, pad)
    xp = F.pad(x, (0, 0, pw, pw, ph, ph))
    if fault == 'left_halo':
        xp[:, :, :pw] = xp[:, :, pw:pw + 1]
    elif fault == 'prev_image_row':
        xp[1:, ph - 1, pw:pw + W] = x[:-1, H - 1]
    elif fault == 'drop_tap':
        w = w.clone()
        w[:, KH - 1, KW // 2, C - 1] = 0
    elif fault == 'swap_kw_c':
        w0, w = w, w.clone()
        w[:, KH // 2, 0, 0], w[:, KH // 2, KW - 1, C - 1] = w0[:, KH // 2, KW - 1, C - 1], w0[:, KH // 2, 0, 0]
    else:
        assert fault is None, fault
    out = x.new_zeros(B, Ho, Wo, Co)
    for kh in range(KH):
        for kw in range(KW):
            out += xp[:, kh:kh + sh * (Ho - 1) + 1:sh, kw:kw + sw * (Wo - 1) + 1:sw] @ w[:, kh, kw].T
    return out.reshape(B * Ho * Wo, Co)


# conv3x3_c64_kernel: output tiles of 8 rows x 32 columns (halo 10 x 34), 2 channel halves x 4 row
# pairs of waves, 16-column sub-tiles.  (1,1,1): every halo pixel but the centre is padding; (1,5,7)
# below a tile; (1,8,32) one tile; (1,9,33) four tiles, the ragged ones 1 wide and 1 high; (1,2,17)
# the sub-tile boundary; (3,17,65) batch boundaries (a halo row of image b +- 1, a column of the row before)
C3_SHAPES = [(1, 1, 1), (1, 5, 7), (1, 8, 32), (1, 9, 33), (1, 2, 17), (3, 17, 65)]
C3_MULTI_TILE = (1, 9, 33)                  # the smallest multi-tile case; with a batch: C3_SHAPES[-1]
C3_LDC_SHAPE = (3, 17, 65)                  # written into the first 64 of 96 channels
C3_EPILOGUES = {'plain': (False, False), 'scale_bias': (True, False), 'relu': (False, True), 'full': (True, True)}


def c3_persistent_shape(cus=256):
    """(B, 20, 70): 3 x 3 ragged tiles per image, B the least with more than 2 * cus tiles -- the grid is
    one workgroup per CU, so some walk three tiles (both halo buffers reused, the vmcnt(4) wait)."""
    return (2 * cus) // 9 + 1, 20, 70


# stem_conv_kernel / stem_img_kernel: output tiles of 4 conv rows x 64 conv columns, a 512-wide grid.
# (1,8,128) exactly one tile; (1,9,129) ragged in both directions; (1,16,126) / (1,15,125) the same
# 8 x 63 map from an even and an odd image (the bottom and right padding differ)
STEM_SHAPES = [(1, 1, 1), (1, 9, 7), (1, 8, 128), (1, 9, 129), (2, 7, 130), (1, 16, 126), (1, 15, 125)]
STEM_MULTI_TILE = (1, 9, 129)               # with a batch: (2, 7, 130)
# 6 tiles (and, pooled at seg_tiles = 1, 6 work units) per image: 1026 > 2 * 512, a workgroup walks three
STEM_PERSISTENT = (171, 18, 130)
# stem_pool_kernel: strips of 62 conv = 31 pooled columns.  Widths: Wo = 61 and 62 (Wp = 31, one strip),
# 63 and 64 (Wp = 32: the second strip has one pooled column), 125 and 150 (test_stem_pool_gpu's);
# heights: Ho = 4, 5, 8, 9 (one tile; a ragged second; two; a ragged third -- with seg_tiles 1 and 2 the
# carried conv row and the pre step are both taken).  Alternately one and two images.
POOL_SHAPES = [(1 + (i + j) % 2, H, W) for i, W in enumerate((122, 124, 125, 127, 250, 300))
               for j, H in enumerate((7, 10, 16, 17))]
POOL_SEG_TILES = (0, 1, 2, 3)
POOL_BIAS1_SHAPE = (2, 17, 250)             # bias = 1 on every channel: padded conv rows / columns would win a border maximum
POOL_ZERO_SHAPE = (1, 10, 127)              # all weights and biases zero
FRONT_RESEED = {}                           # (kind, shape, variant) -> seed offset, where a draw missed exact_headroom


def stem_out(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _front_seed(kind, shape, cls, variant):
    B, H, W = shape
    return ((1 if kind == 'stem' else 2) * 1000003 + B * 7919 + H * 131 + W + (0 if cls == 'exact' else 5)
            + 17 * len(variant or '') + 100 * FRONT_RESEED.get((kind, shape, variant), 0))


@functools.lru_cache(maxsize=6)
def front_case(kind, shape, cls, dtype=None, variant=None, dev='cpu'):
    """One case of either family (the exact class does not depend on dtype: pass None).
      x      what the entry point is given: 'c3' (B, H, W, 64) holding `dtype` values; 'stem' the f32 NCHW
             image -- exact class: exact_x, the in-kernel rounding is the identity; generic: randn NOT yet
             rounded, the reference rounds it to `dtype` as torch does (to nearest even);
      w      OIHW, f32 holding `dtype` values;   scale, bias (64,) f32
      acc, absprod  (B*Ho*Wo, 64) f64 on the CPU: the convolution of the rounded operands and of their
             absolute values, computed on `dev`.
    variant (stem, exact class): 'bias1' -- bias 1 on every channel; 'zero' -- all weights and biases 0."""
    k, stride, pad, Cin, K = FRONT_GEO[kind]
    B, H, W = shape
    g = torch.Generator().manual_seed(_front_seed(kind, shape, cls, variant))
    xshape = (B, H, W, 64) if kind == 'c3' else (B, 3, H, W)
    if cls == 'exact':
        x, w = exact_x(xshape, g), exact_w((64, Cin, k, k), K, g)
        scale, bias = exact_epilogue(64, g)
        xr = x
    else:
        assert variant is None
        xr, w = generic_operands(xshape, (64, Cin, k, k), K, dtype, g)
        x = xr
        if kind == 'stem':          # the kernel is given the unrounded draw of the same generator state
            x = torch.randn(xshape, generator=torch.Generator().manual_seed(_front_seed(kind, shape, cls, variant)))
            assert torch.equal(x.to(dtype).float(), xr)
        scale, bias = generic_epilogue(64, g)
    if variant == 'bias1':
        bias = torch.ones(64)
    elif variant == 'zero':
        w, bias = torch.zeros_like(w), torch.zeros(64)
    xn = (xr if kind == 'c3' else xr.permute(0, 2, 3, 1)).to(dev)
    wn = w.permute(0, 2, 3, 1).to(dev)
    Ho, Wo = out_size(H, W, k, k, stride, pad)
    return {'x': x, 'w': w, 'scale': scale, 'bias': bias, 'K': K, 'B': B, 'Ho': Ho, 'Wo': Wo,
            'acc': conv_taps64(xn, wn, stride, pad).cpu(), 'absprod': conv_taps64(xn.abs(), wn.abs(), stride, pad).cpu()}


def front_expected(case, scale_bias=True, relu=True):
    """(f64 value before the output rounding, the bound's majorant, the scale the bound carries)."""
    s, b = (case['scale'], case['bias']) if scale_bias else (None, None)
    return epilogue64(case['acc'], s, b, None, relu) + (s,)


def pool_rows(v, B, Ho, Wo):
    """torch's 3x3 / stride 2 / pad 1 max_pool2d of the (B*Ho*Wo, C) rows of an NHWC map -> (B*Hp*Wp, C)
    (in f64 for a 16-bit v: the maximum of exactly held values)."""
    t = v.double().reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)
    return F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, v.shape[-1]).to(v.dtype)


def front_exact_cases(cus=256):
    """(kind, shape, variant) of every exact-class case of the GPU module."""
    out = [('c3', s, None) for s in C3_SHAPES + [c3_persistent_shape(cus)]]
    out += [('stem', s, None) for s in STEM_SHAPES + [STEM_PERSISTENT] + POOL_SHAPES]
    return out + [('stem', POOL_BIAS1_SHAPE, 'bias1'), ('stem', POOL_ZERO_SHAPE, 'zero')]
