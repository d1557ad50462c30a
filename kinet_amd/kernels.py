"""Thin torch-tensor front-end over the kinet_amd C-ABI (include/*.h).

Every function launches hand-written HIP kernels from libkinet_amd.so on the current
stream; nothing here falls back to a torch/CPU implementation.  Weights stay torch
Parameters (reference layout, so state_dicts load unchanged); converted copies (dtype
casts, OIHW->OHWI conv packing, folded FrozenBatchNorm) are cached per parameter
version.
"""
import ctypes
import functools
import weakref

import torch

from kinet_amd import _native as N

_cache = {}   # id(tensor) -> (weakref(tensor), {tag: ((version, data_ptr), value)})


def _drop(key):
    def cb(ref, _c=_cache):
        ent = _c.get(key) if _c is not None else None
        if ent is not None and ent[0] is ref:   # a newer tensor may have reused the id
            del _c[key]
    return cb


def cached(t, tag, make):
    """Cache make(t) per tensor object (identity-keyed and weakly held, so a freed
    temporary never aliases a new tensor at the same address), invalidated by in-place
    updates (_version)."""
    if t is None:
        return None
    key = id(t)
    ent = _cache.get(key)
    if ent is None or ent[0]() is not t:
        ent = (weakref.ref(t, _drop(key)), {})
        _cache[key] = ent
    slot = ent[1]
    hit = slot.get(tag)
    ver = (t._version, t.data_ptr())
    if hit is not None and hit[0] == ver:
        return hit[1]
    v = make(t)
    slot[tag] = (ver, v)
    return v


def clear_cache():
    _cache.clear()


def cache_values():
    """Strong references to every cached value (HIP-graph recordings keep them allocated)."""
    return [hit[1] for ent in list(_cache.values()) for hit in ent[1].values()]


def cached_multi(tensors, tag, make):
    """Cache make(*tensors) on the first tensor, invalidated if ANY of them changes."""
    t0 = tensors[0]
    key = id(t0)
    ent = _cache.get(key)
    if ent is None or ent[0]() is not t0:
        ent = (weakref.ref(t0, _drop(key)), {})
        _cache[key] = ent
    ver = tuple((t._version, t.data_ptr()) for t in tensors)
    hit = ent[1].get(tag)
    if hit is not None and hit[0] == ver:
        return hit[1]
    v = make(*tensors)
    ent[1][tag] = (ver, v)
    return v


def set_solo_launch(on):
    """Launch-fill policy of the library (include/kinet_gemm.h kinet_set_solo_launch): True when
    the caller keeps ONE batch in flight (latency mode: partial-round shapes run smaller tiles
    that fill the chip alone), False (default) when several streams overlap.  Outputs are the
    same bit for bit either way.  Returns the previous policy."""
    return bool(N.lib().kinet_set_solo_launch(1 if on else 0))


def param_rows(p, start, end):
    """A stable (cached) row-slice view of a parameter, so its dtype cast is cached too."""
    return cached(p, ('rows', start, end), lambda t: t.detach()[start:end])


def param_matrix(p):
    """Conv 1x1 weight (O, I, 1, 1) viewed as a (O, I) GEMM operand (stable object)."""
    return cached(p, 'matrix', lambda t: t.detach().reshape(t.shape[0], -1))


def weight_as(w, dtype):
    return cached(w, ('w', dtype), lambda t: t.detach().to(dtype).contiguous())


def f32(t):
    return None if t is None else cached(t, 'f32', lambda x: x.detach().float().contiguous())


# ----------------------------------------------------------------------------------- GEMM
def ksplit_for(M, Nout, K, ln=False):
    """Split-K factor for long-K problems with too few output tiles to fill the CUs twice
    over (include/kinet_gemm.h kinet_gemm_ksplit); 1 = no split."""
    return N.lib().kinet_gemm_ksplit(M, Nout, K, 1 if ln else 0)


GEMM_FAMILIES = ('none', 'tiled', 'tiled-dma', 'dma8', 'rw', 'rw_conv', 'conv3x3', 'stem', 'splitk')


def _kernel_id(v):
    return GEMM_FAMILIES[v >> 20], (v >> 10) & 1023, v & 1023


def gemm_last_kernel():
    """(family, bm, bn) of the kernel that served this thread's last GEMM / convolution call
    (include/kinet_gemm.h kinet_gemm_last_kernel); bm = bn = 0 for the special-cased kernels."""
    return _kernel_id(N.lib().kinet_gemm_last_kernel())


GEMM_RW_CONFIG_FIELDS = ('KC', 'NT', 'BMR', 'NS', 'NW', 'OCC', 'HAS_R', 'LN', 'HAS_A2', 'CR', 'PREP', 'out_bytes',
                         'P', 'ng', 'n_mtiles')


def gemm_rw_last_config():
    """The resident-weight kernel instantiation and grid of this thread's last launch as a dict over
    GEMM_RW_CONFIG_FIELDS (include/kinet_gemm.h kinet_gemm_rw_last_config); all zeros when the last
    GEMM / convolution call ran another kernel."""
    out = (ctypes.c_int * len(GEMM_RW_CONFIG_FIELDS))()
    N.call('kinet_gemm_rw_last_config', ctypes.addressof(out))
    return dict(zip(GEMM_RW_CONFIG_FIELDS, out))


def gemm_rw_grid_cap(max_p):
    """Bound the resident-weight kernel's grid.x for this thread (0 = no bound; include/kinet_gemm.h
    kinet_gemm_rw_grid_cap): same outputs bit for bit.  Returns the previous bound."""
    return N.lib().kinet_gemm_rw_grid_cap(int(max_p))


def gemm_plan(M, Nout, K, dtype_code=1, conv=False, Cin=0, ln=False, a2=False, kchunk=0, hm_rows=0, cus=256):
    """The launches the tiled GEMM / convolution kernel plans for a problem under this thread's
    flags and forced tile (include/kinet_gemm.h kinet_gemm_plan; needs no GPU): a list of
    ((family, bm, bn), first row, row tiles).  dtype_code: a kinet_dtype (1 = bf16)."""
    n, out = ctypes.c_int(0), (ctypes.c_int * 6)()
    N.call('kinet_gemm_plan', M, Nout, K, Cin, int(conv), int(ln), int(a2), kchunk, hm_rows, dtype_code, cus,
           ctypes.addressof(n), ctypes.addressof(out))
    return [(_kernel_id(out[3 * i]), out[3 * i + 1], out[3 * i + 2]) for i in range(n.value)]


# the problem fields of kinet_gemm_rw_plan, in the order of include/kinet_gemm.h's KINET_RWP_ enum
GEMM_RW_PROBLEM_FIELDS = ('kind', 'M', 'N', 'K', 'in_dtype', 'out_dtype', 'residual', 'ln', 'a2', 'ldc', 'ldr', 'c_aligned',
                          'r_aligned', 'a2_aligned', 'hm_rows', 'hm_d', 'hm_split', 'hm_d2', 'Cin', 'KW', 'stride', 'stride_w',
                          'pad', 'pad_w', 'Win', 'Wout', 'row_mask')
GEMM_RW_KINDS = ('gemm', 'conv', 'records')


def gemm_rw_plan(M, Nout, K, in_dtype=1, out_dtype=None, kind='gemm', cus=256, **fields):
    """The resident-weight launch planned for a described problem under this thread's flags and grid
    cap (include/kinet_gemm.h kinet_gemm_rw_plan; needs no GPU): None when the kernel does not take
    the problem, else the record gemm_rw_last_config() would return after the launch.  in_dtype /
    out_dtype: kinet_dtypes (1 = bf16; out_dtype defaults to in_dtype, f16 for records); fields: the
    other GEMM_RW_PROBLEM_FIELDS (default: ldc = ldr = N, every pointer aligned, everything else 0)."""
    if out_dtype is None:
        out_dtype = N.dtype_code(torch.float16) if kind == 'records' else in_dtype
    p = dict.fromkeys(GEMM_RW_PROBLEM_FIELDS, 0)
    p.update(kind=GEMM_RW_KINDS.index(kind), M=M, N=Nout, K=K, in_dtype=in_dtype, out_dtype=out_dtype, ldc=Nout, ldr=Nout,
             c_aligned=1, r_aligned=1, a2_aligned=1)
    unknown = set(fields) - set(GEMM_RW_PROBLEM_FIELDS)
    if unknown:
        raise TypeError(f'gemm_rw_plan: unknown fields {sorted(unknown)}')
    p.update({k: int(v) for k, v in fields.items()})
    prob = (ctypes.c_int * len(GEMM_RW_PROBLEM_FIELDS))(*(p[f] for f in GEMM_RW_PROBLEM_FIELDS))
    ok, out = ctypes.c_int(0), (ctypes.c_int * len(GEMM_RW_CONFIG_FIELDS))()
    N.call('kinet_gemm_rw_plan', ctypes.addressof(prob), cus, ctypes.addressof(ok), ctypes.addressof(out))
    return dict(zip(GEMM_RW_CONFIG_FIELDS, out)) if ok.value else None


@functools.lru_cache(maxsize=None)
def _min_a2_rows():
    return N.lib().kinet_gemm_rw_min_a2_rows()


def _epilogue_operand(r, ld):
    """A residual the fused epilogue can read 4 elements at a time (include/kinet_gemm.h "C / R
    alignment"): a view that starts off a 4-element boundary with a row stride that is a multiple
    of 4 is copied (a misaligned out= view cannot be fixed up here: the launcher refuses it)."""
    if ld % 4 == 0 and r.data_ptr() % (4 * r.element_size()):
        return r.contiguous() if not r.is_contiguous() else r.clone()
    return r


KINET_F32_X3 = 4   # include/kinet_common.h


def mm_code(dt):
    """Input dtype code of a GEMM / convolution: f32 operands follow
    torch.get_float32_matmul_precision() -- 'highest' (torch's default): exact f32 MFMA;
    'high' / 'medium': three bf16 MFMA passes per product (KINET_F32_X3, ~2^-17 relative
    error per product; torch's own 'high' mode is this same bf16x3 split or TF32)."""
    if dt == torch.float32 and torch.get_float32_matmul_precision() != 'highest':
        return KINET_F32_X3
    return N.dtype_code(dt)


def linear(x, weight, bias=None, relu=False, residual=None, row_mask=None, out_dtype=None,
           scale=None, out=None, x_add=None, ln=None):
    """y = LN?(relu?((x [+ x_add]) @ W^T * scale + bias + residual)); rows with row_mask -> 0.
    x (..., K) in bf16/f16/f32; weight (Nout, K) any float dtype (cast+cached);
    ln = (gamma, beta, eps) fuses the post-norm LayerNorm over each output row."""
    N.require_gpu(x)
    K = x.shape[-1]
    lead = x.shape[:-1]
    if x_add is not None and x_add.dim() == x.dim() and x_add.shape != x.shape:
        x_add = x_add.expand(x.shape)   # a frame-shared operand (forward_flat's unpadded pos)
    x2 = x.reshape(-1, K)
    kp = (-K) % 8
    if kp:
        # the GEMM's K must be 8-aligned (16-byte K chunks): zero-pad the inputs (KineT's
        # 4 / 1 / 20 / 5 input features); the padded weight copy is cached
        x2 = torch.nn.functional.pad(x2, (0, kp))
        if x_add is not None:
            x_add = torch.nn.functional.pad(x_add.reshape(-1, K), (0, kp))
        K += kp
    elif x2.stride(-1) != 1 or (x2.stride(0) % 8) or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    a2 = None
    if x_add is not None:
        a2 = x_add.reshape(-1, K)
        if a2.stride() != x2.stride() or a2.data_ptr() % 16:
            x2, a2 = x2.contiguous(), a2.contiguous()
            if a2.stride() != x2.stride():
                raise RuntimeError('linear: x_add must match x layout')
    M = x2.shape[0]
    if kp:
        w = cached(weight, ('w_padk', x.dtype, kp),
                   lambda t: torch.nn.functional.pad(t.detach().to(x.dtype), (0, kp)).contiguous())
    else:
        w = weight_as(weight, x.dtype)
    Nout = w.shape[0]
    odt = out_dtype or x.dtype
    if out is None:
        out = torch.empty((M, Nout), dtype=odt, device=x.device)
        ldc = Nout
    else:
        ldc = out.stride(0)
    r = None
    ldr = 0
    if residual is not None:
        r = residual.reshape(-1, Nout)
        if r.stride(-1) != 1:
            r = r.contiguous()
        if r.dtype != odt:
            r = r.to(odt)
        r = _epilogue_operand(r, r.stride(0))
        ldr = r.stride(0)
    mask = None
    if row_mask is not None:
        mask = row_mask.reshape(-1).to(torch.uint8).contiguous()
    e = x.element_size()
    g, b, eps = (f32(ln[0]), f32(ln[1]), float(ln[2])) if ln is not None else (None, None, 0.0)
    work = {'family': 'gemm', 'flops': 2.0 * M * Nout * K, 'shape': (M, Nout, K),
            'bytes': (M * K + Nout * K) * e + M * Nout * out.element_size() * (2 if r is not None else 1)}
    ks = ksplit_for(M, Nout, K, ln is not None) if a2 is None else 1
    if ks > 1:
        ws = torch.empty(ks * M * Nout, dtype=torch.float32, device=x.device)
        N.call('kinet_gemm_splitk', N.ptr(x2), N.ptr(w), N.ptr(out), M, Nout, K, x2.stride(0), K, ldc,
               mm_code(x.dtype), N.ptr(f32(scale)), N.ptr(f32(bias)), N.ptr(r), ldr, int(relu),
               N.ptr(g), N.ptr(b), eps, N.dtype_code(odt), N.ptr(mask), N.ptr(ws), ks, N.stream(x.device),
               work=work)
        return out.view(*lead, Nout) if out.is_contiguous() else out
    N.call('kinet_gemm_ex', N.ptr(x2), N.ptr(a2), N.ptr(w), N.ptr(out), M, Nout, K, x2.stride(0), K, ldc,
           mm_code(x.dtype), N.ptr(f32(scale)), N.ptr(f32(bias)), N.ptr(r), ldr, int(relu),
           N.ptr(g), N.ptr(b), eps, N.dtype_code(odt), N.ptr(mask), N.stream(x.device), work=work)
    return out.view(*lead, Nout) if out.is_contiguous() else out


def ffn_supported(x, linear1, linear2):
    """The fused FFN kernel covers the 16-bit compute modes at d_model 256 / 288."""
    D = x.shape[-1]
    F_ = linear1.weight.shape[0]
    return (x.dtype in (torch.bfloat16, torch.float16) and D in (256, 288) and F_ % 32 == 0
            and linear1.bias is not None and linear2.bias is not None)


def ffn_pack(w1, w2, dtype):
    """kinet_ffn_pack of (W1 (F, D), W2 (D, F)), cached per parameter version."""
    def make(a, b):
        F_, D = a.shape
        a16 = a.detach().to(dtype).contiguous()
        b16 = b.detach().to(dtype).contiguous()
        out = torch.empty(2 * D * F_, dtype=dtype, device=a.device)
        N.call('kinet_ffn_pack', N.ptr(a16), N.ptr(b16), N.ptr(out), D, F_, N.dtype_code(dtype), N.stream(a.device))
        return out
    return cached_multi([w1, w2], ('ffn_pack', dtype), make)


def ffn_fused(x, linear1, linear2, norm=None, out=None):
    """y = norm(x + linear2(relu(linear1(x)))) in one launch (deformable_transformer.py:284-288,
    :361-365); the (M, F) hidden tensor stays on chip.  x (..., D) bf16/f16."""
    N.require_gpu(x)
    D = x.shape[-1]
    F_ = linear1.weight.shape[0]
    x2 = x.reshape(-1, D)
    if x2.stride(-1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.shape[0]
    wp = ffn_pack(linear1.weight, linear2.weight, x.dtype)
    if out is None:
        out = torch.empty((M, D), dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or out.stride(-1) != 1 or out.numel() != M * D:
        raise RuntimeError('ffn_fused: out must be a unit-stride (M, D) tensor of the input dtype')
    g, b, eps = (f32(norm.weight), f32(norm.bias), float(norm.eps)) if norm is not None else (None, None, 0.0)
    e = x.element_size()
    work = {'family': 'gemm', 'flops': 4.0 * M * D * F_, 'shape': ('ffn', M, D, F_),
            'bytes': (2 * M * D + 2 * D * F_) * e}
    N.call('kinet_ffn_fused', N.ptr(x2), x2.stride(0), N.ptr(wp), N.ptr(f32(linear1.bias)), N.ptr(f32(linear2.bias)),
           N.ptr(g), N.ptr(b), eps, N.ptr(out), D, M, D, F_, N.dtype_code(x.dtype), N.stream(x.device), work=work)
    return out.view(*x.shape[:-1], D)


# kinet_ffn_fused takes the 8-wave x 32-row tile from here: kFfnRt2MinRows of csrc/ffn_plan.h
# (tests/test_ffn_plan_cpu.py holds the two together: the plan flips to that tile exactly at this M)
ATTN_OUT_FFN_MIN_ROWS = 16384

# field order of kinet_ffn_launch_plan's plan record (include/kinet_ffn.h, kinet_ffn_plan_field)
FFN_PLAN_FIELDS = ('kernel', 'tiles', 'grid', 'block', 'waves', 'tile_rows', 'wg_tiles', 'wg_per_cu', 'lds')
FFN_KINDS = ('ffn', 'attn_out_ffn', 'pair', 'pair_ds')
FFN_PACK_KINDS = ('ffn', 'pair', 'pair_ds', 'attn_out_ffn')


def ffn_kernel_name(index):
    """Name of entry `index` of the table of instantiations of csrc/ffn_plan.h (no element type), None past its end."""
    name = N.lib().kinet_ffn_kernel_name(int(index))
    return None if name is None else name.decode()


def ffn_launch_plan(kind, M, D, F_=None, DB=None, cus=256):
    """The launch kinet_ffn_fused ('ffn'), kinet_attn_out_ffn_fused ('attn_out_ffn'), kinet_bottleneck_pair
    ('pair') or kinet_bottleneck_pair_ds ('pair_ds') makes for M rows on a device of `cus` compute units
    (kinet_ffn_launch_plan, csrc/ffn_plan.h; no GPU call), under the calling thread's kinet_ffn_set_debug bits
    and the kinet_set_solo_launch policy: a dict of FFN_PLAN_FIELDS with 'kernel' the instantiation's name, or
    None when the entry point refuses D or DB (the message through kinet_last_error)."""
    prob = (ctypes.c_int * 5)(FFN_KINDS.index(kind), int(M), int(D), int(4 * D if F_ is None else F_), int(D if DB is None else DB))
    out = (ctypes.c_int * len(FFN_PLAN_FIELDS))()
    if N.lib().kinet_ffn_launch_plan(ctypes.cast(prob, ctypes.c_void_p), int(cus), ctypes.cast(out, ctypes.c_void_p)) != 0:
        return None
    plan = dict(zip(FFN_PLAN_FIELDS, out))
    plan['kernel'] = ffn_kernel_name(plan['kernel'])
    return plan


def ffn_grid_cap(max_wgs):
    """Bound the grid of the fused FFN / bottleneck-pair launches of the calling thread (0 = none;
    kinet_ffn_grid_cap): same outputs bit for bit.  Returns the previous bound."""
    return N.lib().kinet_ffn_grid_cap(int(max_wgs))


def ffn_last_kernel():
    """Name of the kernel the calling thread's last ffn_fused / attn_out_ffn_fused / bottleneck_pair /
    bottleneck_pair_ds call launched (kinet_ffn_last_kernel), None before the first."""
    return ffn_kernel_name(N.lib().kinet_ffn_last_kernel())


def ffn_pack_map(kind, D, F_, DB=None):
    """The layout of a packed weight stream (kinet_ffn_pack_map, ffn_pack_src of csrc/ffn_plan.h): an int32
    (elements, 3) CPU tensor of (source matrix in the pack call's argument order, row, column) per packed
    element, for kind 'ffn' (ffn_pack), 'attn_out_ffn' (attn_out_ffn_pack), 'pair' (bottleneck_pack) or
    'pair_ds' (bottleneck_pack_ds)."""
    DB = D if DB is None else DB
    n = {'ffn': 2 * D * F_, 'attn_out_ffn': D * D + 2 * D * F_, 'pair': (D + DB) * F_, 'pair_ds': (2 * D + DB) * F_}[kind]
    out = torch.empty((n, 3), dtype=torch.int32)
    N.call('kinet_ffn_pack_map', FFN_PACK_KINDS.index(kind), D, F_, DB, out.data_ptr())
    return out


def attn_out_ffn_supported(x, out_proj, linear1, linear2):
    """The out-projection + LayerNorm pre-phase exists on the 8-wave x 32-row FFN tile only:
    16-bit compute modes, d_model 256, every bias present, and enough rows (x: (..., D)) for
    launch_ffn to pick that tile.  Looks at shapes and dtypes only."""
    D = x.shape[-1]
    M = x.numel() // D if D else 0
    F_ = linear1.weight.shape[0]
    return (x.dtype in (torch.bfloat16, torch.float16) and D == 256 and tuple(out_proj.weight.shape) == (D, D)
            and F_ % 32 == 0 and M >= ATTN_OUT_FFN_MIN_ROWS and out_proj.bias is not None
            and linear1.bias is not None and linear2.bias is not None)


def attn_out_ffn_pack(wo, w1, w2, dtype):
    """kinet_ffn_pack_attn of (Wo (D, D), W1 (F, D), W2 (D, F)), cached per parameter version."""
    def make(o, a, b):
        F_, D = a.shape
        o16 = o.detach().to(dtype).contiguous()
        a16 = a.detach().to(dtype).contiguous()
        b16 = b.detach().to(dtype).contiguous()
        out = torch.empty(D * D + 2 * D * F_, dtype=dtype, device=a.device)
        N.call('kinet_ffn_pack_attn', N.ptr(o16), N.ptr(a16), N.ptr(b16), N.ptr(out), D, F_, N.dtype_code(dtype),
               N.stream(a.device))
        return out
    return cached_multi([wo, w1, w2], ('attn_out_ffn_pack', dtype), make)


def attn_out_ffn_fused(samp, out_proj, residual, norm1, linear1, linear2, norm2, out=None, force=False):
    """y = norm2(x + linear2(relu(linear1(x)))) with x = norm1(residual + out_proj(samp)) in one
    launch (deformable_transformer.py:290-299 after the sampler): x is rounded to the 16-bit type
    once, after norm1, and stays on chip.  samp, residual (..., D) bf16/f16; norm2 may be None.
    force=True skips the row-count gate (the kernel is correct for any M; tests)."""
    N.require_gpu(samp, residual)
    if not force and not attn_out_ffn_supported(samp, out_proj, linear1, linear2):
        raise RuntimeError('attn_out_ffn_fused: unsupported shape / dtype (see attn_out_ffn_supported)')
    D = samp.shape[-1]
    F_ = linear1.weight.shape[0]

    def rows(t):
        t2 = t.reshape(-1, D)
        if t2.stride(-1) != 1 or t2.stride(0) % 8 or t2.data_ptr() % 16:
            t2 = t2.contiguous()
        return t2
    a2, r2 = rows(samp), rows(residual)
    if r2.dtype != samp.dtype or r2.shape != a2.shape:
        raise RuntimeError('attn_out_ffn_fused: residual must match samp in shape and dtype')
    M = a2.shape[0]
    wp = attn_out_ffn_pack(out_proj.weight, linear1.weight, linear2.weight, samp.dtype)
    if out is None:
        out = torch.empty((M, D), dtype=samp.dtype, device=samp.device)
    elif out.dtype != samp.dtype or out.stride(-1) != 1 or out.numel() != M * D:
        raise RuntimeError('attn_out_ffn_fused: out must be a unit-stride (M, D) tensor of the input dtype')
    if norm1 is None or out_proj.bias is None:
        raise RuntimeError('attn_out_ffn_fused: the out-projection bias and norm1 are required')
    g2, b2, eps2 = (f32(norm2.weight), f32(norm2.bias), float(norm2.eps)) if norm2 is not None else (None, None, 0.0)
    e = samp.element_size()
    work = {'family': 'gemm', 'flops': 4.0 * M * D * F_ + 2.0 * M * D * D, 'shape': ('ffn', M, D, F_, 'attn_out'),
            'bytes': (3 * M * D + D * D + 2 * D * F_) * e}
    N.call('kinet_attn_out_ffn_fused', N.ptr(a2), a2.stride(0), N.ptr(r2), r2.stride(0), N.ptr(wp),
           N.ptr(f32(out_proj.bias)), N.ptr(f32(norm1.weight)), N.ptr(f32(norm1.bias)), float(norm1.eps),
           N.ptr(f32(linear1.bias)), N.ptr(f32(linear2.bias)), N.ptr(g2), N.ptr(b2), eps2, N.ptr(out), D, M, D, F_,
           N.dtype_code(samp.dtype), N.stream(samp.device), work=work)
    return out.view(*samp.shape[:-1], D)


def _headmajor_out(out, shape, dtype):
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError(f'out: a contiguous, 16-byte aligned {dtype} tensor of shape {tuple(shape)} expected')
    return out


def value_proj_headmajor(x, weight, bias, head_dim, row_mask=None, out_dtype=None, out=None):
    """MSDA value projection written head-major: x (B, S, K) -> (Nout/head_dim, B, S, head_dim),
    padding rows zeroed (ms_deform_attn.py:64-67).  out_dtype: x.dtype, or float16 from bf16
    operands (the sampling kernel's mixed f16 x f32 FMA path).  out: the tensor to write (tests)."""
    N.require_gpu(x)
    B, S, K = x.shape
    x2 = x.reshape(B * S, K)
    if x2.stride(-1) != 1 or (x2.stride(0) % 8) or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    w = weight_as(weight, x.dtype)
    Nout = w.shape[0]
    od = out_dtype or x.dtype
    shape = (Nout // head_dim, B, S, head_dim)
    out = torch.empty(shape, dtype=od, device=x.device) if out is None else _headmajor_out(out, shape, od)
    mask = row_mask.reshape(-1).to(torch.uint8).contiguous() if row_mask is not None else None
    e = x.element_size()
    N.call('kinet_gemm_headmajor', N.ptr(x2), N.ptr(w), N.ptr(out), B * S, Nout, K, x2.stride(0), K,
           N.dtype_code(x.dtype), N.dtype_code(od), N.ptr(f32(bias)), N.ptr(mask), S, head_dim, N.stream(x.device),
           work={'family': 'gemm', 'flops': 2.0 * B * S * Nout * K, 'shape': (B * S, Nout, K),
                 'bytes': (B * S * K + Nout * K + B * S * Nout) * e})
    return out


class SplitValue:
    """A head_dim-36 MSDA value in the two head-major planes of kinet_gemm_headmajor_split:
    main (M, B, S, 32) and tail (M, B, S, 4), views of one buffer."""
    __slots__ = ('main', 'tail')

    def __init__(self, main, tail):
        self.main, self.tail = main, tail

    @property
    def shape(self):
        M_, B, S, _ = self.main.shape
        return (M_, B, S, 36)

    @property
    def dtype(self):
        return self.main.dtype

    @property
    def device(self):
        return self.main.device

    def dim(self):
        return 4

    def merged(self):
        """(M, B, S, 36) head-major copy (tests / the generic kernel)."""
        return torch.cat([self.main, self.tail], -1)


def split_value_weights(weight, bias, heads):
    """value_proj rows reordered [every head's channels 0-31 | every head's channels 32-35] (the
    split GEMM's column order), cached per parameter version."""
    D = weight.shape[0] // heads

    def perm(t):
        t = t.detach().view(heads, D, *t.shape[1:])
        return torch.cat([t[:, :32].reshape(heads * 32, *t.shape[2:]), t[:, 32:].reshape(heads * (D - 32), *t.shape[2:])],
                         0).contiguous()
    return cached(weight, 'split_w', perm), cached(bias, 'split_b', lambda b: perm(b).float().contiguous())


def value_proj_headmajor_split(x, weight_split, bias_split, heads, row_mask=None, out_dtype=None, out=None):
    """MSDA value projection of a head_dim-36 layer into the two planes the split encoder
    kernel reads (kinet_gemm_headmajor_split): x (B, S, K), weight/bias from split_value_weights
    -> SplitValue(main (heads, B, S, 32), tail (heads, B, S, 4)); padding rows zeroed
    (ms_deform_attn.py:64-67).  out: the flat B*S*Nout buffer to write both planes into (tests)."""
    N.require_gpu(x)
    B, S, K = x.shape
    x2 = x.reshape(B * S, K)
    if x2.stride(-1) != 1 or (x2.stride(0) % 8) or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    w = weight_as(weight_split, x.dtype)
    Nout = w.shape[0]
    od = out_dtype or x.dtype
    buf = torch.empty(B * S * Nout, dtype=od, device=x.device) if out is None else _headmajor_out(out, (B * S * Nout,), od)
    main = buf[:heads * B * S * 32].view(heads, B, S, 32)
    tail = buf[heads * B * S * 32:].view(heads, B, S, Nout // heads - 32)
    mask = row_mask.reshape(-1).to(torch.uint8).contiguous() if row_mask is not None else None
    e = x.element_size()
    N.call('kinet_gemm_headmajor_split', N.ptr(x2), N.ptr(w), N.ptr(buf), B * S, Nout, K, x2.stride(0), K,
           N.dtype_code(x.dtype), N.dtype_code(od), N.ptr(f32(bias_split)), N.ptr(mask), S, 32, heads * 32,
           Nout // heads - 32, N.stream(x.device),
           work={'family': 'gemm', 'flops': 2.0 * B * S * Nout * K, 'shape': (B * S, Nout, K),
                 'bytes': (B * S * K + Nout * K + B * S * Nout) * e})
    return SplitValue(main, tail)


# ----------------------------------------------------------------------------------- conv
def pack_conv_weight(w, dtype, cin_pad=None):
    """OIHW -> OHWI (Cin fastest), optional zero channel padding, cast."""
    def make(t):
        o, i, kh, kw = t.shape
        p = t.detach().permute(0, 2, 3, 1)
        if cin_pad and cin_pad > i:
            p = torch.nn.functional.pad(p, (0, cin_pad - i))
        return p.to(dtype).contiguous()
    return cached(w, ('conv', dtype, cin_pad), make)


def pack_stem_weight(w, dtype, cg):
    """OIHW (Cout, 3, KH, KW) -> (Cout, KH, 1, cg) with w'[o][kh][0][kw*3 + c] = w[o][c][kh][kw]:
    the weights of the tap-folded stem convolution over pack_image_kwfold's layout."""
    def make(t):
        o, i, kh, kw = t.shape
        p = t.detach().permute(0, 2, 3, 1).reshape(o, kh, 1, kw * i)
        p = torch.nn.functional.pad(p, (0, cg - kw * i))
        return p.to(dtype).contiguous()
    return cached(w, ('stem', dtype, cg), make)


def conv2d_nhwc(x, w_packed, stride, pad, scale=None, bias=None, relu=False, residual=None, out=None, ksplit=None):
    """x (B, H, W, Cin) NHWC contiguous; w_packed (Cout, KH, KW, Cin); returns (B, Ho, Wo, Cout).
    stride / pad: int or (vertical, horizontal)."""
    B, H, W, Cin = x.shape
    Cout, KH, KW, Cin2 = w_packed.shape
    if Cin2 != Cin:
        raise RuntimeError(f'conv2d: weight Cin {Cin2} != input Cin {Cin}')
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    Ho = (H + 2 * ph - KH) // sh + 1
    Wo = (W + 2 * pw - KW) // sw + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    ldy = out.stride(2) if out.dim() == 4 else out.stride(-2)
    r = None
    if residual is not None:
        r = _epilogue_operand(residual, Cout)
    e = x.element_size()
    work = {'family': 'conv', 'flops': 2.0 * B * Ho * Wo * Cout * KH * KW * Cin,
            'shape': (B, H, W, Cin, Cout, KH, sh),
            'bytes': (B * H * W * Cin + Cout * KH * KW * Cin + B * Ho * Wo * Cout * (2 if r is not None else 1)) * e}
    tail = (mm_code(x.dtype), N.ptr(scale), N.ptr(bias), N.ptr(r), Cout if r is not None else 0, int(relu), ldy)
    if sh != sw or ph != pw:
        if ksplit not in (None, 1):
            raise RuntimeError('conv2d: split-K needs equal strides / pads')
        N.call('kinet_conv2d_ex', N.ptr(x), N.ptr(w_packed), N.ptr(out), B, H, W, Cin, Ho, Wo, Cout, KH, KW,
               sh, sw, ph, pw, *tail, N.stream(x.device), work=work)
        return out
    args = (N.ptr(x), N.ptr(w_packed), N.ptr(out), B, H, W, Cin, Ho, Wo, Cout, KH, KW, sh, ph) + tail
    ks = ksplit_for(B * Ho * Wo, Cout, KH * KW * Cin) if ksplit is None else ksplit
    if ks > 1:
        ws = torch.empty(ks * B * Ho * Wo * Cout, dtype=torch.float32, device=x.device)
        N.call('kinet_conv2d_splitk', *args, N.ptr(ws), ks, N.stream(x.device), work=work)
    else:
        N.call('kinet_conv2d', *args, N.stream(x.device), work=work)
    return out


def stem_conv_image(img, w_packed, scale, bias, dtype):
    """ResNet stem (7x7/2 conv + folded BN + ReLU) straight from the f32 NCHW image
    (kinet_stem_conv_image): (B, 3, H, W) -> (B, (H-1)//2+1, (W-1)//2+1, 64) NHWC in dtype.
    w_packed: pack_stem_weight(conv1.weight, dtype, 24)."""
    img = img.float().contiguous()
    N.require_gpu(img)
    B, C, H, W = img.shape
    if C != 3:
        raise RuntimeError('stem_conv_image expects 3-channel images')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, 64), dtype=dtype, device=img.device)
    work = {'family': 'conv', 'flops': 2.0 * B * Ho * Wo * 64 * 147, 'shape': ('stem', B, H, W),
            'bytes': B * 3 * H * W * 4 + B * Ho * Wo * 64 * y.element_size()}
    N.call('kinet_stem_conv_image', N.ptr(img), N.ptr(w_packed), N.ptr(f32(scale)), N.ptr(f32(bias)), N.ptr(y),
           B, H, W, N.dtype_code(dtype), N.stream(img.device), work=work)
    return y


def stem_pool_image(img, w_packed, scale, bias, dtype, seg_tiles=0):
    """stem_conv_image + maxpool_3x3s2 in one launch (kinet_stem_pool_image): (B, 3, H, W) ->
    (B, Hp, Wp, 64) NHWC in dtype, Hp = ((H-1)//2)//2 + 1 (Wp alike), bit-identical to the two
    launches.  seg_tiles: 4-row conv tiles per work unit (0 = the launcher's choice)."""
    img = img.float().contiguous()
    N.require_gpu(img)
    B, C, H, W = img.shape
    if C != 3:
        raise RuntimeError('stem_pool_image expects 3-channel images')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    y = torch.empty((B, Hp, Wp, 64), dtype=dtype, device=img.device)
    work = {'family': 'conv', 'flops': 2.0 * B * Ho * Wo * 64 * 147, 'shape': ('stem_pool', B, H, W),
            'bytes': B * 3 * H * W * 4 + B * Hp * Wp * 64 * y.element_size()}
    N.call('kinet_stem_pool_image', N.ptr(img), N.ptr(w_packed), N.ptr(f32(scale)), N.ptr(f32(bias)), N.ptr(y),
           B, H, W, N.dtype_code(dtype), int(seg_tiles), N.stream(img.device), work=work)
    return y


def bottleneck_pack(w3, w1, s3, s1, dtype):
    """kinet_bottleneck_pack of conv3 (F, D, 1, 1) and the next block's conv1 (DB, F, 1, 1) with
    their FrozenBN scales folded in, cached per parameter version."""
    def make(a, b, sa, sb):
        F_, D, DB = a.shape[0], a.shape[1], b.shape[0]
        a32 = a.detach().reshape(F_, D).float().contiguous()
        b32 = b.detach().reshape(DB, F_).float().contiguous()
        out = torch.empty((D + DB) * F_, dtype=dtype, device=a.device)
        N.call('kinet_bottleneck_pack', N.ptr(a32), N.ptr(b32), N.ptr(f32(sa)), N.ptr(f32(sb)), N.ptr(out), D, F_, DB,
               N.dtype_code(dtype), N.stream(a.device))
        return out
    return cached_multi([w3, w1, s3, s1], ('bneck_pack', dtype), make)


def bottleneck_pair_supported(dtype, w3, w1):
    """The fused pair covers 16-bit NHWC rows with D = planes in {64, 128, 256}, F = 4 D (conv3
    weight (F, D, 1, 1)) and the next conv1 (DB, F, 1, 1) with DB = D, or DB = 128 at D = 64."""
    F_, D, DB = w3.shape[0], w3.shape[1], w1.shape[0]
    return (dtype in (torch.bfloat16, torch.float16) and D in (64, 128, 256) and F_ == 4 * D
            and (DB == D or (D == 64 and DB == 128))
            and tuple(w3.shape) == (F_, D, 1, 1) and tuple(w1.shape) == (DB, F_, 1, 1))


def bottleneck_pair(x, residual, packed, b3, b1):
    """ResNet bottleneck pair (kinet_bottleneck_pair): x = block i's conv2 output (B, H, W, D)
    NHWC, residual (B, H, W, F) -> (y, t): y = relu(conv3(x) * s3 + b3 + residual) (the block
    output, F = 4 D channels), t = relu(conv1'(y) * s1 + b1) (the next block's conv1 output,
    DB = b1.numel() channels); the BN scales are in `packed` (bottleneck_pack)."""
    N.require_gpu(x)
    B, H, W, D = x.shape
    F_ = 4 * D
    if residual.shape != (B, H, W, F_) or not residual.is_contiguous() or residual.dtype != x.dtype:
        raise RuntimeError('bottleneck_pair: residual must be a contiguous (B, H, W, 4D) tensor of the input dtype')
    M = B * H * W
    DB = b1.numel()
    y = torch.empty((B, H, W, F_), dtype=x.dtype, device=x.device)
    t = torch.empty((B, H, W, DB), dtype=x.dtype, device=x.device)
    e = x.element_size()
    work = {'family': 'conv', 'flops': 2.0 * M * F_ * (D + DB), 'shape': ('bneck', M, D, F_, DB),
            'bytes': (M * D + 2 * M * F_ + M * DB + (D + DB) * F_) * e}
    N.call('kinet_bottleneck_pair', N.ptr(x), D, N.ptr(residual), N.ptr(packed), N.ptr(f32(b3)), N.ptr(f32(b1)),
           N.ptr(y), N.ptr(t), M, D, F_, DB, N.dtype_code(x.dtype), N.stream(x.device), work=work)
    return y, t


def bottleneck_pack_ds(w3, wds, w1, s3, sds, s1, b3, bds, dtype):
    """kinet_bottleneck_pack_ds of stage 1's block-0 conv3 (256, 64, 1, 1), its downsample conv
    (256, 64, 1, 1) and block 1's conv1 (64, 256, 1, 1) with their FrozenBN scales folded in ->
    (packed weights, b3 + b_ds in f32), cached per parameter version."""
    def make(a, d, b, sa, sd, sb, ba, bd):
        F_, D, DB = a.shape[0], a.shape[1], b.shape[0]
        a32 = a.detach().reshape(F_, D).float().contiguous()
        d32 = d.detach().reshape(F_, D).float().contiguous()
        b32 = b.detach().reshape(DB, F_).float().contiguous()
        out = torch.empty((2 * D + DB) * F_, dtype=dtype, device=a.device)
        N.call('kinet_bottleneck_pack_ds', N.ptr(a32), N.ptr(d32), N.ptr(b32), N.ptr(f32(sa)), N.ptr(f32(sd)),
               N.ptr(f32(sb)), N.ptr(out), D, F_, DB, N.dtype_code(dtype), N.stream(a.device))
        return out, (ba.detach().float() + bd.detach().float()).contiguous()
    return cached_multi([w3, wds, w1, s3, sds, s1, b3, bds], ('bneck_pack_ds', dtype), make)


def bottleneck_pair_ds_supported(dtype, w3, wds, w1):
    """The downsample-folded pair covers stage 1 only: 16-bit rows, conv3 (256, 64, 1, 1), the
    downsample conv (256, 64, 1, 1) over a 64-channel block input, the next conv1 (64, 256, 1, 1)."""
    return (dtype in (torch.bfloat16, torch.float16) and tuple(w3.shape) == (256, 64, 1, 1)
            and tuple(wds.shape) == (256, 64, 1, 1) and tuple(w1.shape) == (64, 256, 1, 1))


def bottleneck_pair_ds(x, x0, packed, b3ds, b1):
    """Stage 1's first bottleneck pair with block 0's downsample folded in
    (kinet_bottleneck_pair_ds): x = block 0's conv2 output (B, H, W, 64), x0 = the block input
    (B, H, W, 64) -> (y, t): y = relu(conv3(x) * s3 + conv_ds(x0) * s_ds + b3ds) (256 channels),
    t = relu(conv1'(y) * s1 + b1) (64 channels); packed, b3ds from bottleneck_pack_ds."""
    N.require_gpu(x, x0)
    B, H, W, D = x.shape
    if D != 64 or x0.shape != x.shape or x0.dtype != x.dtype or not x.is_contiguous() or not x0.is_contiguous():
        raise RuntimeError('bottleneck_pair_ds: x and x0 must be contiguous (B, H, W, 64) tensors of one dtype')
    if b3ds.numel() != 256 or b3ds.dtype != torch.float32 or b1.numel() != 64:
        raise RuntimeError('bottleneck_pair_ds: b3ds must be 256 f32 values and b1 64 values')
    M, F_, DB = B * H * W, 256, 64
    y = torch.empty((B, H, W, F_), dtype=x.dtype, device=x.device)
    t = torch.empty((B, H, W, DB), dtype=x.dtype, device=x.device)
    e = x.element_size()
    work = {'family': 'conv', 'flops': 2.0 * M * F_ * (D + 64 + DB), 'shape': ('bneck_ds', M, D, F_, DB),
            'bytes': (M * D + M * 64 + M * F_ + M * DB + (D + 64 + DB) * F_) * e}
    N.call('kinet_bottleneck_pair_ds', N.ptr(x), D, N.ptr(x0), 64, N.ptr(packed), N.ptr(b3ds), N.ptr(f32(b1)),
           N.ptr(y), N.ptr(t), M, D, F_, DB, N.dtype_code(x.dtype), N.stream(x.device), work=work)
    return y, t


def maxpool_3x3s2(x):
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    N.call('kinet_maxpool2d_3x3s2', N.ptr(x), N.ptr(y), B, H, W, C, N.dtype_code(x.dtype), N.stream(x.device))
    return y


def pack_image(img, dtype, cpad=8):
    """(B, 3, H, W) f32 NCHW -> (B, H, W, cpad) NHWC dtype."""
    img = img.float().contiguous()
    B, C, H, W = img.shape
    if C != 3:
        raise RuntimeError('pack_image expects 3-channel images')
    y = torch.empty((B, H, W, cpad), dtype=dtype, device=img.device)
    N.call('kinet_pack_image_nhwc', N.ptr(img), N.ptr(y), B, H, W, cpad, N.dtype_code(dtype), N.stream(img.device))
    return y


def pack_image_kwfold(img, dtype, kw, stride, pad, cg):
    """(B, 3, H, W) f32 NCHW -> (B, H, Wo, cg) with the kw horizontal taps of a stride-`stride`
    filter folded into channels (kinet_pack_image_kwfold)."""
    img = img.float().contiguous()
    B, C, H, W = img.shape
    if C != 3:
        raise RuntimeError('pack_image_kwfold expects 3-channel images')
    Wo = (W + 2 * pad - kw) // stride + 1
    y = torch.empty((B, H, Wo, cg), dtype=dtype, device=img.device)
    N.call('kinet_pack_image_kwfold', N.ptr(img), N.ptr(y), B, H, W, kw, stride, pad, cg, N.dtype_code(dtype),
           N.stream(img.device), work={'family': 'kinet_pack_image_kwfold'})
    return y


# ------------------------------------------------------------------------------ norms
def layernorm(x, weight, bias, eps=1e-5, residual=None, out=None):
    d = x.shape[-1]
    x2 = x.contiguous()
    r = residual.contiguous() if residual is not None else None
    y = out if out is not None else torch.empty_like(x2)
    rows = x2.numel() // d
    N.call('kinet_layernorm', N.ptr(x2), N.ptr(r), N.ptr(f32(weight)), N.ptr(f32(bias)), N.ptr(y), rows, d,
           float(eps), N.dtype_code(x.dtype), 0, N.stream(x.device),
           work={'family': 'norm', 'bytes': rows * d * x2.element_size() * (3 if r is not None else 2)})
    return y


def groupnorm_nhwc(x, weight, bias, groups, eps=1e-5, out=None, out_batch_stride=None):
    """x (B, HW, C) contiguous -> out rows at out + b*out_batch_stride (default packed)."""
    B, HW, C = x.shape
    if out is None:
        out = torch.empty_like(x)
        out_batch_stride = HW * C
    nws = N.lib().kinet_groupnorm_workspace(B, HW, C, groups, N.dtype_code(x.dtype))
    stats = torch.empty(max(1, nws), dtype=torch.float32, device=x.device)
    N.call('kinet_groupnorm', N.ptr(x), N.ptr(f32(weight)), N.ptr(f32(bias)), N.ptr(out), B, HW, C, groups,
           int(out_batch_stride), float(eps), N.dtype_code(x.dtype), N.ptr(stats), N.stream(x.device),
           work={'family': 'norm', 'bytes': 2 * x.numel() * x.element_size()})
    return out


def add(a, b, out=None):
    a = a.contiguous()
    b = b.contiguous()
    y = out if out is not None else torch.empty_like(a)
    N.call('kinet_add', N.ptr(a), N.ptr(b), N.ptr(y), a.numel(), N.dtype_code(a.dtype), N.stream(a.device),
           work={'family': 'eltwise', 'bytes': 3 * a.numel() * a.element_size()})
    return y


# ---------------------------------------------------------------- position embedding
def sine_position_embed(mask, dim_t, num_pos_feats, three_d=False, frame=0, frames=1, normalize=True, scale=1.0,
                        level_embed=None, out=None, out_batch_stride=None, out_dtype=torch.float32):
    """Sine embedding of a padding mask (B, H, W) as NHWC rows (kinet_sine_position_embed):
    returns (B, H*W, C) (or writes rows into `out` at out + b*out_batch_stride)."""
    N.require_gpu(mask)
    B, H, W = mask.shape
    C = (3 if three_d else 2) * num_pos_feats
    if out is None:
        out = torch.empty((B, H * W, C), dtype=out_dtype, device=mask.device)
        out_batch_stride = H * W * C
    m = mask.to(torch.uint8).contiguous()
    N.call('kinet_sine_position_embed', N.ptr(m), N.ptr(dim_t), N.ptr(f32(level_embed) if level_embed is not None
                                                                          else None),
           N.ptr(out), B, H, W, num_pos_feats, int(three_d), frame, frames, int(normalize), float(scale),
           int(out_batch_stride), N.dtype_code(out.dtype), N.stream(mask.device),
           work={'family': 'pos_embed', 'bytes': B * H * W * C * out.element_size()})
    return out


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms semantics on the GPU: indices of the kept boxes, by descending score
    (ties by index).  boxes (n, 4) xyxy, scores (n)."""
    N.require_gpu(boxes, scores)
    n = boxes.shape[0]
    keep = torch.zeros(n, dtype=torch.uint8, device=boxes.device)
    if n:
        b = boxes.float().contiguous()
        s = scores.float().contiguous()
        N.call('kinet_nms', N.ptr(b), N.ptr(s), N.ptr(keep), n, float(iou_threshold), N.stream(boxes.device))
        idx = keep.nonzero().flatten()
        # descending, ties by index, NaN first: the kernel's own rank order
        return idx[torch.sort(s[idx], descending=True, stable=True)[1]]
    return keep.nonzero().flatten()


# --------------------------------------------------------------------------- attention
_SEED_POOL = {}     # device index -> [seeds tensor, next index, generator state key after the draw]
_SEED_BLOCK = 64


def _gen_key(gen):
    return (gen.initial_seed(), gen.get_offset())


def dropout_seed(device):
    """A device int64 seed for the dropout kernels, drawn from torch's generator of `device`
    (as F.dropout draws its Philox offset from it), without a host sync.  Seeds are drawn 64 at
    a time (one launch instead of one per dropout site); the block is redrawn whenever the
    generator has moved since the draw (torch.manual_seed, other random ops), so a reseeded
    run replays the same seeds."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    ent = _SEED_POOL.get(idx)
    if ent is None or ent[1] >= _SEED_BLOCK or ent[2] != _gen_key(gen):
        seeds = torch.randint(0, 2 ** 62, (_SEED_BLOCK,), dtype=torch.int64, device=torch.device('cuda', idx))
        ent = _SEED_POOL[idx] = [seeds, 0, _gen_key(gen)]
    s = ent[0][ent[1]:ent[1] + 1]
    ent[1] += 1
    return s


def dropout_mask(seed, n, p):
    """The keep mask (uint8, n elements) the dropout kernels derive from `seed` at probability p."""
    keep = torch.empty(n, dtype=torch.uint8, device=seed.device)
    N.call('kinet_dropout_mask', N.ptr(seed), n, float(p), N.ptr(keep), N.stream(seed.device))
    return keep


# field order of kinet_mha_launch_plan's records (include/kinet_ops.h) and its kernel codes
MHA_PROBLEM_FIELDS = ('dtype', 'head_dim', 'batch', 'heads', 'Lq', 'Lk', 'ldq', 'ldk', 'ldv', 'ldo', 'align', 'dropout',
                      'knob')
MHA_PLAN_FIELDS = ('kernel', 'grid_x', 'grid_y', 'grid_z', 'block', 'lds', 'resident_maxk', 'stream_kt')
MHA_KERNELS = ('fma', 'resident', 'stream')


def mha_launch_plan(dtype, head_dim, batch, heads, Lq, Lk, ld=None, align=16, dropout=False, knob=None):
    """The launch mha_core makes for this problem (kinet_mha_launch_plan, csrc/attn_plan.h; no GPU call): a dict
    of MHA_PLAN_FIELDS with 'kernel' one of MHA_KERNELS.  ld: the row stride of q / k / v / out in elements, one
    value or four (default heads * head_dim); align: bytes every pointer is a multiple of; knob: a
    kinet_mha_set_mfma value (default: the calling thread's)."""
    ld = heads * head_dim if ld is None else ld
    lds = tuple(ld) if isinstance(ld, (tuple, list)) else (ld,) * 4
    prob = (ctypes.c_int * len(MHA_PROBLEM_FIELDS))(N.dtype_code(dtype), head_dim, batch, heads, Lq, Lk, *lds, align,
                                                    int(bool(dropout)), -1 if knob is None else knob)
    out = (ctypes.c_int * len(MHA_PLAN_FIELDS))()
    N.call('kinet_mha_launch_plan', ctypes.cast(prob, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p))
    plan = dict(zip(MHA_PLAN_FIELDS, out))
    plan['kernel'] = MHA_KERNELS[plan['kernel']]
    return plan


def mha_last_kernel():
    """Which of MHA_KERNELS the calling thread's last mha_core call launched (kinet_mha_last_kernel), None
    before the first."""
    code = N.lib().kinet_mha_last_kernel()
    return None if code < 0 else MHA_KERNELS[code]


def __getattr__(name):
    # csrc/attn_plan.h through the library: the 16-bit head_dim 32 / 36 MFMA kernels keep a head's keys resident
    # in LDS up to MHA_RESIDENT_MAXK[head_dim]; longer key sets stream in tiles of MHA_STREAM_KT keys
    if name == 'MHA_RESIDENT_MAXK':
        return {D: mha_launch_plan(torch.bfloat16, D, 1, 1, 1, 1)['resident_maxk'] for D in (32, 36)}
    if name == 'MHA_STREAM_KT':
        return mha_launch_plan(torch.bfloat16, 32, 1, 1, 1, 1)['stream_kt']
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def mha_core(q, k, v, heads, scale, key_mask=None, out=None, dropout_p=0.0, seed=None):
    """q (B, Lq, E) (row stride may exceed E), k/v (B, Lk, E) -> (B, Lq, E).  dropout_p > 0:
    attention-probability dropout with the keep mask of `seed` (kinet_mha_core_dropout).
    No dropout, bf16 / f16, head_dim 32 / 36: the MFMA kernels of csrc/attn.hip (keys resident
    in LDS up to MHA_RESIDENT_MAXK, streamed above); everything else the FMA kernel."""
    B, Lq, E = q.shape
    Lk = k.shape[1]
    D = E // heads
    for t in (q, k, v):
        if t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise RuntimeError('mha_core: rows must be unit-stride with packed batches')
    o = out if out is not None else torch.empty((B, Lq, E), dtype=q.dtype, device=q.device)
    km = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    if dropout_p > 0:
        N.call('kinet_mha_core_dropout', N.ptr(q), q.stride(1), N.ptr(k), k.stride(1), N.ptr(v), v.stride(1),
               N.ptr(o), o.stride(1), B, Lq, Lk, heads, D, float(scale), N.dtype_code(q.dtype), N.ptr(km),
               float(dropout_p), N.ptr(seed), N.stream(q.device),
               work={'family': 'attn', 'flops': 4.0 * B * heads * Lq * Lk * D})
        return o
    N.call('kinet_mha_core', N.ptr(q), q.stride(1), N.ptr(k), k.stride(1), N.ptr(v), v.stride(1), N.ptr(o),
           o.stride(1), B, Lq, Lk, heads, D, float(scale), N.dtype_code(q.dtype), N.ptr(km), N.stream(q.device),
           work={'family': 'attn', 'flops': 4.0 * B * heads * Lq * Lk * D})
    return o


def box_refine(tmp, ref, valid_ratios=None, want_input=True, out=None):
    """tmp (B, Q, 4) f32, ref (B, Q, 2|4) f32 -> new_ref (B, Q, 4) [, ref_input (B, Q, L, 4)];
    out: optional contiguous (B, Q, 4) f32 destination of new_ref."""
    B, Q, _ = tmp.shape
    tmp = tmp.float().contiguous()
    ref = ref.float().contiguous()
    nref = out if out is not None else torch.empty((B, Q, 4), dtype=torch.float32, device=tmp.device)
    rin = None
    L = 0
    if want_input:
        vr = valid_ratios.float().contiguous()
        L = vr.shape[1]
        rin = torch.empty((B, Q, L, 4), dtype=torch.float32, device=tmp.device)
    else:
        vr = None
    N.call('kinet_box_refine', N.ptr(tmp), N.ptr(ref), ref.shape[-1], N.ptr(vr), N.ptr(nref), N.ptr(rin), B, Q, L,
           N.stream(tmp.device))
    return nref, rin


# ------------------------------------------------------------- two-stage proposal stage
TOPK_MAX_K = 1024   # include/kinet_two_stage.h


def two_stage_proposals(shapes, mask, batch, device):
    """gen_encoder_output_proposals' shape / mask part (kinet_two_stage_proposals): shapes the
    host list of level (H, W); mask (B, S) bool / uint8 or None -> (proposals (B, S, 4) f32 in
    logit space, +inf on padded / out-of-range rows; keep (B, S) uint8)."""
    import ctypes
    shapes = [(int(h), int(w)) for h, w in shapes]
    S = sum(h * w for h, w in shapes)
    m = None
    if mask is not None:
        N.require_gpu(mask)
        m = mask.reshape(batch, S).to(torch.uint8).contiguous()
    prop = torch.empty((batch, S, 4), dtype=torch.float32, device=device)
    keep = torch.empty((batch, S), dtype=torch.uint8, device=device)
    hw = (ctypes.c_int * (2 * len(shapes)))(*[v for s in shapes for v in s])
    N.call('kinet_two_stage_proposals', hw, len(shapes), N.ptr(m), N.ptr(prop), N.ptr(keep), batch, S,
           N.stream(device))
    return prop, keep


def topk_rows(scores, k):
    """Indices (rows, k) int64 of the k largest entries of each row of an f32 matrix, read in
    place through its strides (e.g. channel 0 of (B, S, C) logits): descending, NaN first, ties
    by ascending index == torch.sort(descending=True, stable=True)[1][:, :k].  No host sync."""
    N.require_gpu(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise RuntimeError('topk_rows: scores must be a 2-d float32 matrix')
    rows, S = scores.shape
    out = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    N.call('kinet_topk_rows', N.ptr(scores), scores.stride(0), scores.stride(1), rows, S, int(k), N.ptr(out),
           N.stream(scores.device), work={'family': 'topk', 'bytes': 4 * rows * S * 4})
    return out


_proposal_dim_t = {}


def proposal_dim_t(device):
    """get_proposal_pos_embed's dim_t (deformable_transformer.py:82-83), evaluated with torch on
    the host as the reference does; one table per device."""
    device = torch.device(device)
    t = _proposal_dim_t.get(device)
    if t is None:
        d = torch.arange(128, dtype=torch.float32)
        d = 10000 ** (2 * torch.div(d, 2, rounding_mode='floor') / 128)
        t = _proposal_dim_t[device] = d.to(device)
    return t


def two_stage_queries(coord_unact, idx, out_dtype, dim_t=None):
    """coord_unact (B, S, 4) f32, idx (B, k) int64 -> (reference_points (B, k, 4) f32 =
    sigmoid(gathered), proposal position embedding (B, k, 512) in out_dtype)."""
    N.require_gpu(coord_unact, idx)
    B, S, _ = coord_unact.shape
    k = idx.shape[1]
    cu = coord_unact.float().contiguous()
    ix = idx.contiguous()
    dim_t = proposal_dim_t(cu.device) if dim_t is None else dim_t
    ref = torch.empty((B, k, 4), dtype=torch.float32, device=cu.device)
    pos = torch.empty((B, k, 512), dtype=out_dtype, device=cu.device)
    N.call('kinet_two_stage_queries', N.ptr(cu), N.ptr(ix), N.ptr(dim_t), N.ptr(ref), N.ptr(pos), B, S, k,
           N.dtype_code(out_dtype), N.stream(cu.device))
    return ref, pos


def two_stage_fill_rows(y, keep, row):
    """In place: y[r] = row for every row r of y (..., d) with keep[r] == 0."""
    N.require_gpu(y, keep, row)
    d = y.shape[-1]
    if not y.is_contiguous() or not keep.is_contiguous() or row.dtype != y.dtype:
        raise RuntimeError('two_stage_fill_rows: contiguous y / keep and a row of the same dtype required')
    N.call('kinet_two_stage_fill_rows', N.ptr(y), N.ptr(keep), N.ptr(row), y.numel() // d, d, N.dtype_code(y.dtype),
           N.stream(y.device))
    return y


def two_stage_boxes(tmp, proposals):
    """(coord_unact = tmp + proposals, boxes = sigmoid(coord_unact)), all (B, S, 4) f32."""
    N.require_gpu(tmp, proposals)
    t = tmp.float().contiguous()
    p = proposals.contiguous()
    unact, boxes = torch.empty_like(p), torch.empty_like(p)
    N.call('kinet_two_stage_boxes', N.ptr(t), N.ptr(p), N.ptr(unact), N.ptr(boxes), p.numel() // 4, N.stream(p.device))
    return unact, boxes


def two_stage_boxes_backward(d_boxes, d_coord_unact, boxes):
    """d_tmp of two_stage_boxes = d_boxes * b (1 - b) + d_coord_unact (either gradient may be None), all
    (..., 4) f32; exactly 0 from the d_boxes term where b == 1 (the +inf proposals)."""
    N.require_gpu(d_boxes, d_coord_unact, boxes)
    if d_boxes is None and d_coord_unact is None:
        raise RuntimeError('two_stage_boxes_backward: both input gradients are None')
    b = boxes.contiguous()
    if b.dtype != torch.float32 or b.shape[-1] != 4:
        raise RuntimeError('two_stage_boxes_backward: boxes must be f32 (..., 4)')
    db = None if d_boxes is None else d_boxes.float().contiguous()
    du = None if d_coord_unact is None else d_coord_unact.float().contiguous()
    if any(t is not None and t.shape != b.shape for t in (db, du)):
        raise RuntimeError('two_stage_boxes_backward: the gradients must have the boxes\' shape')
    out = torch.empty_like(b)
    N.call('kinet_two_stage_boxes_backward', N.ptr(db), N.ptr(du), N.ptr(b), N.ptr(out), b.numel() // 4,
           N.stream(b.device))
    return out


def two_stage_mask_rows(x, keep):
    """y[r] = x[r] where keep[r] else 0 (exactly, whatever the dropped row holds): x (..., d) f32, keep one
    uint8 per row.  Applied to a gradient it is its own backward."""
    N.require_gpu(x, keep)
    d = x.shape[-1]
    if x.dtype != torch.float32 or keep.dtype != torch.uint8 or keep.numel() * d != x.numel():
        raise RuntimeError('two_stage_mask_rows: x must be f32 (..., d) and keep uint8 with one byte per row')
    xc, kc = x.contiguous(), keep.contiguous()
    y = torch.empty_like(xc)
    N.call('kinet_two_stage_mask_rows', N.ptr(xc), N.ptr(kc), N.ptr(y), kc.numel(), d, N.stream(x.device),
           work={'family': 'two_stage', 'bytes': 8 * xc.numel()})
    return y


# --------------------------------------------------- criterion kernels (csrc/criterion.hip)
def match_cost_focal(logits, boxes, tgt_labels, tgt_boxes, tgt_start, w_class, w_bbox, w_giou, alpha=0.25,
                     gamma=2.0, want_check=True):
    """The block-diagonal focal matcher cost (kinet_match_cost_focal): logits (B, Q, C) f32, boxes (B, Q, 4)
    f32 cxcywh, tgt_labels (T) int64, tgt_boxes (T, 4) f32, tgt_start (B + 1) int32 on the device ->
    (cost (Q, T) f32: column j against the Q predictions of the image that owns it; ok: a device bool
    scalar, False when any box is degenerate (util/box_ops.py:44-45), or None)."""
    N.require_gpu(logits, boxes, tgt_labels, tgt_boxes, tgt_start)
    if logits.dtype != torch.float32 or boxes.dtype != torch.float32 or logits.dim() != 3 \
            or tuple(boxes.shape) != tuple(logits.shape[:2]) + (4,):
        raise RuntimeError(f'match_cost_focal: logits must be f32 (B, Q, C) and boxes f32 (B, Q, 4): got '
                           f'{tuple(logits.shape)} {logits.dtype}, {tuple(boxes.shape)} {boxes.dtype}')
    B, Q, C = logits.shape
    T = tgt_labels.numel()
    if tgt_labels.dtype != torch.int64 or tgt_boxes.dtype != torch.float32 or tuple(tgt_boxes.shape) != (T, 4) \
            or tgt_start.dtype != torch.int32 or tgt_start.numel() != B + 1:
        raise RuntimeError('match_cost_focal: tgt_labels int64 (T), tgt_boxes f32 (T, 4) and tgt_start int32 (B + 1) '
                           'required')
    lg, bx, tl, tb, ts = (t.contiguous() for t in (logits, boxes, tgt_labels, tgt_boxes, tgt_start))
    cost = torch.empty((Q, T), dtype=torch.float32, device=logits.device)
    ok = torch.ones((), dtype=torch.uint8, device=logits.device) if want_check else None
    N.call('kinet_match_cost_focal', N.ptr(lg), N.ptr(bx), N.ptr(tl), N.ptr(tb), N.ptr(ts), N.ptr(cost), N.ptr(ok),
           B, Q, C, T, float(w_class), float(w_bbox), float(w_giou), float(alpha), float(gamma),
           N.stream(logits.device), work={'family': 'criterion', 'bytes': 4 * Q * T + 20 * B * Q})
    return cost, (None if ok is None else ok.view(torch.bool))


def _focal_set_args(logits, pos_rows, pos_cls):
    N.require_gpu(logits, pos_rows, pos_cls)
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise RuntimeError(f'focal_set_loss: logits must be f32 (R, C): got {tuple(logits.shape)} {logits.dtype}')
    if pos_rows.dtype != torch.int64 or pos_cls.dtype != torch.int64 or pos_rows.shape != pos_cls.shape \
            or pos_rows.dim() != 1:
        raise RuntimeError('focal_set_loss: pos_rows and pos_cls must be int64 vectors of one length')
    return logits.contiguous(), pos_rows.contiguous(), pos_cls.contiguous()


def focal_set_loss(logits, pos_rows, pos_cls, num_boxes, alpha=0.25, gamma=2.0):
    """sum over (R, C) of the sigmoid focal loss against the sparse positives (pos_rows[i], pos_cls[i]),
    divided by num_boxes (kinet_focal_set_loss) -> a 0-d f32 tensor; two runs are bit-identical."""
    logits, pos_rows, pos_cls = _focal_set_args(logits, pos_rows, pos_cls)
    R, C = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = _ws(N.lib().kinet_focal_set_loss_workspace(R, C), logits.device)
    N.call('kinet_focal_set_loss', N.ptr(logits), N.ptr(pos_rows), N.ptr(pos_cls), N.ptr(loss), R, C,
           pos_rows.numel(), float(alpha), float(gamma), 1.0 / float(num_boxes), N.ptr(ws), N.stream(logits.device),
           work={'family': 'criterion', 'bytes': 4 * logits.numel()})
    return loss[0]


def focal_set_loss_backward(logits, pos_rows, pos_cls, dloss, num_boxes, alpha=0.25, gamma=2.0):
    """dloss * d focal_set_loss / d logits (kinet_focal_set_loss_backward): dloss one f32 on the device."""
    logits, pos_rows, pos_cls = _focal_set_args(logits, pos_rows, pos_cls)
    N.require_gpu(dloss)
    if dloss.dtype != torch.float32 or dloss.numel() != 1:
        raise RuntimeError('focal_set_loss_backward: dloss must be one f32')
    R, C = logits.shape
    dlogits = torch.empty_like(logits)
    N.call('kinet_focal_set_loss_backward', N.ptr(logits), N.ptr(pos_rows), N.ptr(pos_cls), N.ptr(dloss.contiguous()),
           N.ptr(dlogits), R, C, pos_rows.numel(), float(alpha), float(gamma), 1.0 / float(num_boxes),
           N.stream(logits.device), work={'family': 'criterion', 'bytes': 8 * logits.numel()})
    return dlogits


# ------------------------------------------------------------------------------ MSDA
_tile_orders = {}


def encoder_tile_order(shapes, device, qt=16):
    """Processing order of the encoder's 16-query tiles for msda_fused: sorted by the
    normalised image row of each tile's first query, so the tiles of all levels that sample
    the same image band run together and share the value rows in L2 (the natural order
    sweeps the image once per level).  Cached per (shapes, device)."""
    key = (tuple(tuple(int(v) for v in s) for s in shapes), str(device), qt)
    o = _tile_orders.get(key)
    if o is None:
        import numpy as np
        hw = np.array([h * w for h, w in key[0]], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(hw)[:-1]])
        lq = int(hw.sum())
        q = np.arange((lq + qt - 1) // qt, dtype=np.int64) * qt
        lvl = np.searchsorted(starts, q, side='right') - 1
        H = np.array([h for h, _ in key[0]], dtype=np.float64)[lvl]
        W = np.array([w for _, w in key[0]], dtype=np.int64)[lvl]
        y = ((q - starts[lvl]) // W + 0.5) / H
        o = torch.as_tensor(np.argsort(y, kind='stable').astype(np.int32), device=device)
        _tile_orders[key] = o
    return o


_host_shapes = {}
_enc_plans = {}
# template-argument spelling of the element types in rocprofv3 kernel names
_KT = {torch.bfloat16: 'kinet::bf16_t', torch.float16: 'kinet::f16_t', torch.float32: 'float', torch.float64: 'double'}


def msda_fused_last_kernel():
    """The forward sampling kernel the calling thread's last msda_fused / msda_encoder* call
    launched (kinet_msda_fused_last_kernel): ('generic', vec), ('fast', L), ('encoder', fl, front
    end) with front end 'offlog', 'records' or 'split', or None (no launch)."""
    code = N.lib().kinet_msda_fused_last_kernel()
    if code < 0:
        return None
    fam, det = code >> 8, code & 255
    if fam == 3:
        return ('encoder', det & 15, 'split' if det & 32 else 'records' if det & 16 else 'offlog')
    return ({1: 'generic', 2: 'fast'}[fam], det)


def msda_encoder_set_strips(strips):
    """Strips per head map for the encoder sampler on the calling thread (0 = the plan's own
    choice; kinet_msda_encoder_set_strips, A/B tooling).  The cached plans are dropped, so
    msda_encoder_plan reports what the next launch runs.  Returns the previous value."""
    old = N.lib().kinet_msda_encoder_set_strips(int(strips))
    _enc_plans.clear()
    return old


def msda_encoder_plan(shapes, batch, n_heads, Lq, channels=32):
    """kinet_msda_encoder_plan_ex for host level shapes: (levels gathered from HBM, strips per head
    map, LDS map pixels used, workgroups), or None when no strip plan fits the LDS map.  Cached."""
    key = (tuple(tuple(int(v) for v in s) for s in shapes), int(batch), int(n_heads), int(Lq), int(channels))
    if key not in _enc_plans:
        import ctypes
        hs = (ctypes.c_int64 * 8)(*[v for s in key[0] for v in s])
        out = (ctypes.c_int32 * 4)()
        rc = N.lib().kinet_msda_encoder_plan_ex(ctypes.cast(hs, ctypes.c_void_p), key[1], key[2], key[3], key[4],
                                                ctypes.cast(out, ctypes.c_void_p))
        _enc_plans[key] = tuple(out) if rc == 0 else None
    return _enc_plans[key]


# field order of kinet_msda_launch_plan's plan record (include/kinet_msda.h, kinet_msda_plan_field)
MSDA_PLAN_FIELDS = ('family', 'vec', 'fused', 'l', 'nj', 'sp', 'pow2', 'aln', 'sg', 'grid_x', 'grid_y', 'grid_z', 'block',
                    'lds', 'qt', 'lpq', 'na', 'QT', 'MH', 'QP', 'qc', 'log2ns', 'blocked', 'head_bytes', 'last')
MSDA_FAMILIES = ('none', 'msda_fwd_kernel', 'msda_fused_kernel', 'msda_fused_fast_kernel', 'msda_bwd_list_kernel',
                 'msda_bwd_kernel')
MSDA_BWD_LAST = {1: 'msda_bwd_list_kernel', 0: 'msda_bwd_kernel'}   # kinet_msda_backward_last_kernel codes
_launch_plans = {}


def msda_launch_plan(kind, N_, S, M_, D, L, Lq, P_, value_dtype, out_dtype=None, loc_dtype=None, strides=(0, 0, 0),
                     value_align=0, tune=(0, 0, 0, 0, 0), debug=0, cus=256):
    """The launch kinet_msda_forward ('forward'), kinet_msda_fused_forward ('fused') or kinet_msda_backward
    ('backward') makes for this problem (kinet_msda_launch_plan, csrc/msda_plan.h; no GPU call): a dict of
    MSDA_PLAN_FIELDS with 'family' the kernel's name, or None when the entry point refuses it (the message
    through kinet_last_error).  dtypes as torch dtypes; strides = value (sb, ss, sm) in elements; tune = the
    arguments of kinet_msda_backward_tune.  Cached."""
    loc_dtype = loc_dtype or (value_dtype if value_dtype in (torch.float32, torch.float64) else torch.float32)
    key = (kind, N_, S, M_, D, L, Lq, P_, value_dtype, out_dtype or value_dtype, loc_dtype, tuple(strides),
           value_align, tuple(tune), debug, cus)
    if key not in _launch_plans:
        f = [('forward', 'fused', 'backward').index(kind), N_, S, M_, D, L, Lq, P_, N.dtype_code(value_dtype),
             N.dtype_code(out_dtype or value_dtype), N.dtype_code(loc_dtype), *strides, value_align, *tune, debug]
        prob = (ctypes.c_int64 * len(f))(*[int(v) for v in f])
        out = (ctypes.c_int32 * len(MSDA_PLAN_FIELDS))()
        rc = N.lib().kinet_msda_launch_plan(ctypes.cast(prob, ctypes.c_void_p), int(cus), ctypes.cast(out, ctypes.c_void_p))
        plan = None
        if rc == 0:
            plan = dict(zip(MSDA_PLAN_FIELDS, out))
            plan['family'] = MSDA_FAMILIES[plan['family']]
        _launch_plans[key] = plan
    return _launch_plans[key]


def _template_name(kernel, args, defaults):
    """`kernel<args>` as rocprofv3 prints an instantiation: trailing arguments at their defaults dropped."""
    args = list(args)
    while defaults and args[-1] == defaults[-1]:
        args, defaults = args[:-1], defaults[:-1]
    return '%s<%s>' % (kernel, ', '.join(str(a).lower() if isinstance(a, bool) else str(a) for a in args))


def msda_fused_kernel_name(plan, value_dtype, out_dtype, offlog_dtype):
    """work['kernel'] of an msda_fused call from its launch plan."""
    if plan is None or plan['family'] == 'none':
        return 'none'
    if plan['family'] == 'msda_fused_fast_kernel':
        # template <T, TO, TL, L, P, MH = 4, SG = 4>
        return _template_name(plan['family'], [_KT[value_dtype], _KT[out_dtype], _KT[offlog_dtype], plan['l'], 4,
                                               plan['MH'], plan['sg']], [4, 4])
    return '%s<%s, *>' % (plan['family'], _KT[value_dtype])


def msda_encoder_kernel_name(out_dtype, fl, ref_dim, masked, front):
    """work['kernel'] of an encoder sampler call: msda_enc_kernel<TO, FL, REFD, QM, REC = false, TAIL = false,
    NW = 16> for the plan's gathered levels `fl` and the front end ('offlog', 'records' or 'split', as
    msda_fused_last_kernel names them; the split kernel runs 12 waves)."""
    rec, tail = front == 'records', front == 'split'
    return _template_name('msda_enc_kernel', [_KT[out_dtype], fl, 2 if rec else ref_dim, bool(masked) and not rec, rec,
                                              tail, 12 if tail else 16], [False, False, 16])


# head_dim-36 encoder calls through the split value planes + kinet_msda_encoder_forward_split
# when eligible; False keeps the generic fused kernel on the (M, B, S, 36) value (A/B and tests)
MSDA_SPLIT = [True]


def msda_split_supported(dtype, head_dim, shapes, Lq, n_heads, n_levels, n_points, batch):
    """True when a head_dim-36 encoder call runs on the strip kernel with the split value planes:
    16-bit compute, 4 levels x 4 points, >= 2048 queries per frame, a strip plan for 72-byte
    pixels and a tail plane below 2^28 bytes."""
    if not MSDA_SPLIT[0] or dtype not in (torch.bfloat16, torch.float16) or head_dim != 36:
        return False
    if n_levels != 4 or n_points != 4 or Lq < 2048 or shapes is None or len(shapes) != 4:
        return False
    S = sum(int(h) * int(w) for h, w in shapes)
    if batch * Lq >= (1 << 24) or S * 8 >= (1 << 28):
        return False
    return msda_encoder_plan(shapes, batch, n_heads, Lq, 36) is not None


def msda_encoder_split(value, shapes, offlog_hm, reference_points, n_heads, query_attn_mask=None, out_dtype=None,
                       query_tile_order=None, out=None):
    """Head_dim-36 encoder sampling (kinet_msda_encoder_forward_split): value a SplitValue from
    value_proj_headmajor_split, offlog_hm (M, B, Lq, 48) f16, reference_points (B, Lq, 4, 2|4) f32
    -> (B, Lq, M*36).  out: the tensor to write (tests)."""
    main, tail = value.main, value.tail
    M_, B, S, _ = main.shape
    D = 36
    Lq = offlog_hm.shape[2]
    key = tuple(tuple(int(v) for v in s) for s in shapes)
    hs = _host_shapes.get(key)
    if hs is None:
        hs = _host_shapes[key] = torch.tensor(key, dtype=torch.int64)
    ref = reference_points.float().contiguous()
    od = out_dtype or torch.bfloat16
    shape = (B, Lq, M_ * D)
    out = torch.empty(shape, dtype=od, device=main.device) if out is None else _headmajor_out(out, shape, od)
    qm = query_attn_mask.to(torch.uint8).contiguous() if query_attn_mask is not None else None
    if query_tile_order is not None and (query_tile_order.dtype != torch.int32 or
                                         query_tile_order.numel() != (Lq + 15) // 16):
        raise RuntimeError('msda_encoder_split: query_tile_order must be int32 with ceil(Lq/16) entries')
    offlog_hm = offlog_hm.contiguous()
    nsamp = B * Lq * M_ * 16
    plan = msda_encoder_plan(key, B, M_, Lq, 36)
    kname = msda_encoder_kernel_name(od, plan[0] if plan else -1, ref.shape[-1], qm is not None, 'split')
    N.call('kinet_msda_encoder_forward_split', N.ptr(main), main.stride(1), main.stride(0), N.ptr(tail),
           tail.stride(1), tail.stride(0), N.ptr(hs), N.ptr(offlog_hm), N.ptr(ref), ref.shape[-1], N.ptr(qm),
           N.ptr(out), B, S, M_, D, 4, Lq, 4, N.dtype_code(od), N.ptr(query_tile_order), N.stream(main.device),
           work={'family': 'msda', 'flops': 10.0 * nsamp * D, 'Lq': Lq, 'S': S, 'kernel': kname,
                 # compulsory bytes: both value planes once, f16 offsets + logits, refs, output once
                 'bytes': B * S * M_ * D * 2 + offlog_hm.numel() * 2 + ref.numel() * 4
                 + out.numel() * out.element_size()})
    return out


def msda_encoder_supported(value, shapes, Lq, n_heads, n_levels, n_points, batch):
    """True when kinet_msda_encoder_forward takes the call: f16 head-major values of head_dim
    32, 4 levels x 4 points, an encoder-sized query set (>= 2048 per frame) and a strip plan
    that fits the LDS map (kinet_msda_encoder_plan)."""
    if value.dim() != 4 or value.dtype != torch.float16 or value.shape[-1] != 32 or value.stride(2) != 32:
        return False
    if n_levels != 4 or n_points != 4 or Lq < 2048 or shapes is None or len(shapes) != 4:
        return False
    if batch * Lq >= (1 << 24) or msda_encoder_plan(shapes, batch, n_heads, Lq) is None:
        return False
    return value.data_ptr() % 16 == 0 and value.stride(1) % 8 == 0 and value.stride(0) % 8 == 0


def _load_add_operand(x2, x_add, B, Lq, K):
    """(x2, a2, a2_rows) for a GEMM over x2 = x.reshape(B*Lq, K) rows with x_add added at load:
    an x_add of ONE frame (1, Lq, K) for a batch of B > 1 frames stays one frame in memory and
    every frame's rows read it (a2_rows = Lq: the unpadded batch's shared position embedding,
    deformable_transformer.py forward_flat) -- else x_add has x's rows and layout."""
    if x_add is None:
        return x2, None, 0
    if x_add.shape[0] == 1 and B > 1 and Lq >= _min_a2_rows():
        if x2.stride(-1) != 1 or x2.stride(0) != K or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        a2 = x_add.reshape(Lq, K)
        if a2.stride() != x2.stride() or a2.data_ptr() % 16:
            a2 = a2.contiguous()
        return x2, a2, Lq
    if x_add.shape[0] != B:
        x_add = x_add.expand(B, Lq, K)
    a2 = x_add.reshape(B * Lq, K)
    if x2.stride(-1) != 1 or (x2.stride(0) % 8) or x2.data_ptr() % 16 or a2.stride() != x2.stride() or \
            a2.data_ptr() % 16:
        x2, a2 = x2.contiguous(), a2.contiguous()
    return x2, a2, 0


def offsets_proj_headmajor(x, weight, bias, heads, x_add=None, out_dtype=torch.float16, out=None):
    """The MSDA offsets + logits projection (x [+ x_add]) @ W^T + b stored head-major
    (heads, B, Lq, Nout/heads): W's rows must already be grouped per head
    (MSDeformAttn.packed_offsets_weights_headmajor).  out: the tensor to write (tests)."""
    N.require_gpu(x)
    B, Lq, K = x.shape
    x2 = x.reshape(B * Lq, K)
    if x_add is None and (x2.stride(-1) != 1 or (x2.stride(0) % 8) or x2.data_ptr() % 16):
        x2 = x2.contiguous()
    x2, a2, a2_rows = _load_add_operand(x2, x_add, B, Lq, K)
    w = weight_as(weight, x.dtype)
    Nout = w.shape[0]
    rec = Nout // heads
    shape = (heads, B, Lq, rec)
    out = torch.empty(shape, dtype=out_dtype, device=x.device) if out is None else _headmajor_out(out, shape, out_dtype)
    e = x.element_size()
    N.call('kinet_gemm_headmajor_ex', N.ptr(x2), N.ptr(a2), N.ptr(w), N.ptr(out), B * Lq, Nout, K, x2.stride(0), K,
           N.dtype_code(x.dtype), N.dtype_code(out_dtype), N.ptr(f32(bias)), None, Lq, rec, a2_rows,
           N.stream(x.device),
           work={'family': 'gemm', 'flops': 2.0 * B * Lq * Nout * K, 'shape': (B * Lq, Nout, K),
                 'role': 'msda_prep',
                 'bytes': (B * Lq * K + (0 if a2 is None else a2.shape[0] * K) + Nout * K) * e + B * Lq * Nout * 2})
    return out


def msda_encoder(value, shapes, offlog_hm, reference_points, n_heads, query_attn_mask=None, out_dtype=None,
                 query_tile_order=None, out=None):
    """Encoder-sized MSDeformAttn sampling (kinet_msda_encoder_forward): value (M, B, S, 32)
    f16 head-major, shapes = host list of (H, W), offlog_hm (M, B, Lq, 48) f16 from
    offsets_proj_headmajor, reference_points (B, Lq, 4, 2|4) f32 -> (B, Lq, M*32).  out: the tensor
    to write (tests)."""
    M_, B, S, D = value.shape
    Lq = offlog_hm.shape[2]
    key = tuple(tuple(int(v) for v in s) for s in shapes)
    hs = _host_shapes.get(key)
    if hs is None:
        hs = _host_shapes[key] = torch.tensor(key, dtype=torch.int64)
    ref = reference_points.float().contiguous()
    od = out_dtype or torch.bfloat16
    shape = (B, Lq, M_ * D)
    out = torch.empty(shape, dtype=od, device=value.device) if out is None else _headmajor_out(out, shape, od)
    qm = query_attn_mask.to(torch.uint8).contiguous() if query_attn_mask is not None else None
    if query_tile_order is not None and (query_tile_order.dtype != torch.int32 or
                                         query_tile_order.numel() != (Lq + 15) // 16):
        raise RuntimeError('msda_encoder: query_tile_order must be int32 with ceil(Lq/16) entries')
    offlog_hm = offlog_hm.contiguous()
    nsamp = B * Lq * M_ * 16
    plan = msda_encoder_plan(key, B, M_, Lq)
    # the instantiation kinet_msda_encoder_forward launches (as rocprofv3 names it)
    kname = msda_encoder_kernel_name(od, plan[0] if plan else -1, ref.shape[-1], qm is not None, 'offlog')
    N.call('kinet_msda_encoder_forward', N.ptr(value), value.stride(1), value.stride(0), N.ptr(hs), N.ptr(offlog_hm),
           N.ptr(ref), ref.shape[-1], N.ptr(qm), N.ptr(out), B, S, M_, D, 4, Lq, 4, N.dtype_code(od),
           N.ptr(query_tile_order), N.stream(value.device),
           work={'family': 'msda', 'flops': 10.0 * nsamp * D, 'Lq': Lq, 'S': S, 'kernel': kname,
                 # compulsory bytes: value once, f16 offsets + logits, refs, output once
                 'bytes': B * S * M_ * D * 2 + offlog_hm.numel() * 2 + ref.numel() * 4 + out.numel() * out.element_size()})
    return out


# encoder calls sample through kinet_msda_sample_records + kinet_msda_encoder_forward_records
# (phase 1 in the projection epilogue) when eligible; False keeps the f16 offsets/logits path
# (A/B and tests)
MSDA_RECORDS = [True]


def msda_record_frac_bits(shapes):
    """Fraction bits of the records' fixed-point locations for these level shapes: the most that
    leave an integer part holding every level's H and W (at most 10), or None (< 6: too large)."""
    mx = max(max(int(h), int(w)) for h, w in shapes)
    ib = max(1, (mx - 1).bit_length())
    fb = min(10, 16 - ib)
    return fb if fb >= 6 else None


def msda_records_supported(query, shapes_host, n_heads, n_levels, n_points):
    return (MSDA_RECORDS[0] and query.dtype in (torch.bfloat16, torch.float16) and query.shape[-1] == 256
            and n_heads % 4 == 0 and n_levels == 4 and n_points == 4 and shapes_host is not None
            and len(shapes_host) == 4 and msda_record_frac_bits(shapes_host) is not None)


def msda_sample_records(x, weight, bias, heads, reference_points, shapes_host, x_add=None, query_attn_mask=None):
    """The encoder MSDA projection with softmax / locations / bilinear setup in the GEMM epilogue
    (kinet_msda_sample_records): x (B, Lq, 256) [+ x_add], W rows grouped (head, level, 12)
    (MSDeformAttn.packed_records_weights), reference_points (B, Lq, 4, 2|4) -> (records
    (heads, B, Lq, 24) int32 = 96 bytes each, frac_bits)."""
    N.require_gpu(x)
    B, Lq, K_ = x.shape
    x2 = x.reshape(B * Lq, K_)
    if x_add is None and (x2.stride(-1) != 1 or (x2.stride(0) % 8) or x2.data_ptr() % 16):
        x2 = x2.contiguous()
    x2, a2, a2_rows = _load_add_operand(x2, x_add, B, Lq, K_)
    w = weight_as(weight, x.dtype)
    key = tuple(tuple(int(v) for v in s) for s in shapes_host)
    hs = _host_shapes.get(key)
    if hs is None:
        hs = _host_shapes[key] = torch.tensor(key, dtype=torch.int64)
    fb = msda_record_frac_bits(key)
    ref = reference_points.float().contiguous()
    qm = query_attn_mask.to(torch.uint8).contiguous() if query_attn_mask is not None else None
    rec = torch.empty((heads, B, Lq, 24), dtype=torch.int32, device=x.device)
    e = x.element_size()
    N.call('kinet_msda_sample_records', N.ptr(x2), N.ptr(a2), N.ptr(w), N.ptr(f32(bias)), B * Lq, heads, K_,
           x2.stride(0), N.dtype_code(x.dtype), N.ptr(ref), ref.shape[-1], N.ptr(qm), N.ptr(hs), 4, 4, fb, N.ptr(rec),
           a2_rows, N.stream(x.device),
           work={'family': 'gemm', 'flops': 2.0 * B * Lq * heads * 48 * K_, 'shape': (B * Lq, heads * 48, K_),
                 'role': 'msda_prep',
                 'bytes': (B * Lq * K_ + (0 if a2 is None else a2.shape[0] * K_) + heads * 48 * K_) * e
                 + ref.numel() * 4 + rec.numel() * 4})
    return rec, fb


def msda_encoder_records(value, shapes, records, frac_bits, out_dtype=None, query_tile_order=None, out=None):
    """Encoder-sized MSDA sampling from sampling records (kinet_msda_encoder_forward_records):
    value (M, B, S, 32) f16 head-major, records (M, B, Lq, 24) int32 from msda_sample_records
    -> (B, Lq, M*32).  out: the tensor to write (tests)."""
    M_, B, S, D = value.shape
    Lq = records.shape[2]
    key = tuple(tuple(int(v) for v in s) for s in shapes)
    hs = _host_shapes.get(key)
    if hs is None:
        hs = _host_shapes[key] = torch.tensor(key, dtype=torch.int64)
    od = out_dtype or torch.bfloat16
    shape = (B, Lq, M_ * D)
    out = torch.empty(shape, dtype=od, device=value.device) if out is None else _headmajor_out(out, shape, od)
    if query_tile_order is not None and (query_tile_order.dtype != torch.int32 or
                                         query_tile_order.numel() != (Lq + 15) // 16):
        raise RuntimeError('msda_encoder_records: query_tile_order must be int32 with ceil(Lq/16) entries')
    records = records.contiguous()
    nsamp = B * Lq * M_ * 16
    plan = msda_encoder_plan(key, B, M_, Lq)
    kname = msda_encoder_kernel_name(od, plan[0] if plan else -1, 2, False, 'records')
    N.call('kinet_msda_encoder_forward_records', N.ptr(value), value.stride(1), value.stride(0), N.ptr(hs),
           N.ptr(records), int(frac_bits), N.ptr(out), B, S, M_, D, 4, Lq, 4, N.dtype_code(od),
           N.ptr(query_tile_order), N.stream(value.device),
           work={'family': 'msda', 'flops': 10.0 * nsamp * D, 'Lq': Lq, 'S': S, 'kernel': kname,
                 # compulsory bytes: value once, the 96-byte records, output once
                 'bytes': B * S * M_ * D * 2 + records.numel() * 4 + out.numel() * out.element_size()})
    return out


def msda_fused(value, spatial_shapes, offlog, reference_points, n_heads, n_levels, n_points,
               query_attn_mask=None, want_loc_attw=False, head_major=False, out_dtype=None,
               query_tile_order=None, out=None):
    """Sampling of MSDeformAttn.forward (ms_deform_attn.py:69-87) in one kernel.
    value: projected values, either (B, S, d) row-major (column slices allowed) or, with
    head_major=True, (M, B, S, D) as written by value_proj_headmajor;
    offlog (B, Lq, M*L*P*3) f32 (or f16 with 16-bit values) [offsets | logits];
    reference_points (B, Lq, L, 2|4) f32.
    out_dtype: value.dtype, or bfloat16 from float16 values (mixed-precision gather path).
    query_tile_order: optional int32 (ceil(Lq/16),) processing order of the 16-query tiles
    (encoder_tile_order); only the fast 16-bit D=32 kernel uses it, the generic kernel
    ignores it (the output is identical either way).
    out: the tensor to write (tests).
    Cached weights/geometry are built on the stream current at first use: a caller that
    runs several streams from a cold start synchronises once after the first forward.
    Returns (B, Lq, d) [, loc, attw]."""
    if head_major:
        M_, B, S, D = value.shape
        if M_ != n_heads:
            raise RuntimeError(f'head-major value has {M_} heads, module expects {n_heads}')
        d = M_ * D
        if value.stride(-1) != 1 or value.data_ptr() % 16:
            value = value.contiguous()
        vsb, vss, vsm = value.stride(1), value.stride(2), value.stride(0)
    else:
        B, S, d = value.shape
        D = d // n_heads
        if not (value.stride(-1) == 1 and value.data_ptr() % 16 == 0):
            value = value.contiguous()
        vsb, vss, vsm = value.stride(0), value.stride(1), D
    Lq = offlog.shape[1]
    offlog = offlog.contiguous()
    ref = reference_points.float().contiguous()
    if ref.shape[2] != n_levels:
        raise RuntimeError(f'reference_points has {ref.shape[2]} levels, module expects {n_levels}')
    od = out_dtype or value.dtype
    out = torch.empty((B, Lq, d), dtype=od, device=value.device) if out is None else _headmajor_out(out, (B, Lq, d), od)
    loc = attw = None
    if want_loc_attw:
        loc = torch.empty((B, Lq, n_heads, n_levels, n_points, 2), dtype=torch.float32, device=value.device)
        attw = torch.empty((B, Lq, n_heads, n_levels, n_points), dtype=torch.float32, device=value.device)
    qm = query_attn_mask.to(torch.uint8).contiguous() if query_attn_mask is not None else None
    if query_tile_order is not None:
        # the kernel reads torder[tile] for every 16-query tile of the grid
        t = query_tile_order
        if (t.dtype != torch.int32 or t.device != value.device or not t.is_contiguous()
                or t.numel() != (Lq + 15) // 16):
            raise RuntimeError(f'msda_fused: query_tile_order must be a contiguous int32 tensor on '
                               f'{value.device} with ceil(Lq/16) = {(Lq + 15) // 16} entries')
    if offlog.dtype not in (torch.float32, torch.float16):
        raise RuntimeError('msda_fused: the offsets/logits projection must be f32 or f16')
    ev = value.element_size()
    nsamp = B * Lq * n_heads * n_levels * n_points
    # the instantiation kinet_msda_fused_forward launches, as rocprofv3 names it
    kname = msda_fused_kernel_name(
        msda_launch_plan('fused', B, S, n_heads, D, n_levels, Lq, n_points, value.dtype, od, offlog.dtype,
                         (vsb, vss, vsm), value.data_ptr() % 16), value.dtype, od, offlog.dtype)
    N.call('kinet_msda_fused_forward', N.ptr(value), vsb, vss, vsm, N.ptr(spatial_shapes), N.ptr(offlog),
           offlog.shape[-1], N.ptr(ref), ref.shape[-1], N.ptr(qm), N.ptr(out), N.ptr(loc), N.ptr(attw), B, S,
           n_heads, D, n_levels, Lq, n_points, N.dtype_code(value.dtype), N.dtype_code(od), N.dtype_code(offlog.dtype),
           N.ptr(query_tile_order), N.stream(value.device),
           work={'family': 'msda', 'flops': 10.0 * nsamp * D,
                 # compulsory bytes: value once, f32 offsets+logits, refs, output once
                 'bytes': B * S * d * ev + nsamp * 3 * offlog.element_size() + ref.numel() * 4
                 + B * Lq * d * out.element_size()
                 + (nsamp * 3 * 4 if want_loc_attw else 0),
                 'Lq': Lq, 'S': S, 'shape': (B, Lq, S), 'kernel': kname})
    if want_loc_attw:
        return out, loc, attw
    return out


# ------------------------------------------------------------------ backward (kinet_grad.h)
def transpose2d(x):
    """(R, C) -> (C, R) contiguous (kinet_transpose)."""
    N.require_gpu(x)
    if x.stride(-1) != 1:
        x = x.contiguous()
    R, C = x.shape
    y = torch.empty((C, R), dtype=x.dtype, device=x.device)
    N.call('kinet_transpose', N.ptr(x), N.ptr(y), R, C, x.stride(0), R, N.dtype_code(x.dtype), N.stream(x.device),
           work={'family': 'grad', 'bytes': 2 * x.numel() * x.element_size()})
    return y


def im2col_nhwc(x, KH, KW, stride, pad):
    """x (B, H, W, C) -> (B*Ho*Wo, KH*KW*C) patch matrix (kinet_im2col_nhwc)."""
    B, H, W, C = x.shape
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    Ho, Wo = (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1
    cols = torch.empty((B * Ho * Wo, KH * KW * C), dtype=x.dtype, device=x.device)
    N.call('kinet_im2col_nhwc', N.ptr(x.contiguous()), N.ptr(cols), B, H, W, C, Ho, Wo, KH, KW, sh, sw, ph, pw,
           N.dtype_code(x.dtype), N.stream(x.device), work={'family': 'grad', 'bytes': 2 * cols.numel() * x.element_size()})
    return cols


def col2im_nhwc(cols, x_shape, KH, KW, stride, pad):
    """Adjoint of im2col_nhwc: (B*Ho*Wo, KH*KW*C) -> (B, H, W, C)."""
    B, H, W, C = x_shape
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    Ho, Wo = (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1
    dx = torch.empty((B, H, W, C), dtype=cols.dtype, device=cols.device)
    N.call('kinet_col2im_nhwc', N.ptr(cols.contiguous()), N.ptr(dx), B, H, W, C, Ho, Wo, KH, KW, sh, sw, ph, pw,
           N.dtype_code(cols.dtype), N.stream(cols.device),
           work={'family': 'grad', 'bytes': (cols.numel() + dx.numel()) * cols.element_size()})
    return dx


def gemm_tn(a, b, out=None, accumulate=False):
    """out (M, N) f32 [+]= a^T b for a (K, M), b (K, N) (kinet_gemm_tn): weight gradients."""
    N.require_gpu(a, b)
    if a.stride(-1) != 1:
        a = a.contiguous()
    if b.stride(-1) != 1:
        b = b.contiguous()
    K_, M = a.shape
    K2, Nn = b.shape
    if K2 != K_ or a.dtype != b.dtype:
        raise RuntimeError('gemm_tn: operand mismatch')
    if out is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=a.device)
    nws = N.lib().kinet_gemm_tn_workspace(M, Nn, K_)
    if accumulate:
        nws = max(nws, M * Nn)
    ws = torch.empty(max(1, nws), dtype=torch.float32, device=a.device) if nws else None
    N.call('kinet_gemm_tn', N.ptr(a), N.ptr(b), N.ptr(out), M, Nn, K_, a.stride(0), b.stride(0), out.stride(0),
           mm_code(a.dtype), int(accumulate), N.ptr(ws), N.stream(a.device),
           work={'family': 'gemm', 'flops': 2.0 * M * Nn * K_, 'shape': ('tn', M, Nn, K_)})
    return out


def colsum(a, out=None, accumulate=False):
    """out[c] (+)= sum_r a[r, c] (f32)."""
    if a.stride(-1) != 1:
        a = a.contiguous()
    R, C = a.shape
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(1, N.lib().kinet_colsum_workspace(R, C)), dtype=torch.float32, device=a.device)
    N.call('kinet_colsum', N.ptr(a), N.ptr(out), R, C, a.stride(0), N.dtype_code(a.dtype), int(accumulate), N.ptr(ws),
           N.stream(a.device), work={'family': 'grad', 'bytes': a.numel() * a.element_size()})
    return out


def layernorm_backward(dy, x, gamma, eps, need_params=True):
    d = x.shape[-1]
    dy2, x2 = dy.reshape(-1, d).contiguous(), x.reshape(-1, d).contiguous()
    rows = x2.shape[0]
    dx = torch.empty_like(x2)
    dg = torch.empty(d, dtype=torch.float32, device=x.device) if need_params else None
    db = torch.empty(d, dtype=torch.float32, device=x.device) if need_params else None
    ws = torch.empty(max(1, N.lib().kinet_layernorm_backward_workspace(rows, d)), dtype=torch.float32, device=x.device)
    N.call('kinet_layernorm_backward', N.ptr(dy2), N.ptr(x2), N.ptr(f32(gamma)), N.ptr(dx), N.ptr(dg), N.ptr(db), rows,
           d, float(eps), N.dtype_code(x.dtype), N.ptr(ws), N.stream(x.device),
           work={'family': 'norm', 'bytes': 3 * x2.numel() * x2.element_size()})
    return dx.view(x.shape), dg, db


def _rows(t, d):
    t = t.reshape(-1, d)
    return t if t.is_contiguous() else t.contiguous()


def dropout_add_layernorm(x, r, weight, bias, eps, p, seed):
    """LayerNorm(x + dropout_p(r)) over the last dim, f32 (kinet_dropout_add_layernorm)."""
    d = x.shape[-1]
    x2, r2 = _rows(x, d), _rows(r, d)
    y = torch.empty_like(x2)
    N.call('kinet_dropout_add_layernorm', N.ptr(x2), N.ptr(r2), N.ptr(f32(weight)), N.ptr(f32(bias)), N.ptr(y),
           x2.shape[0], d, float(eps), float(p), N.ptr(seed), N.stream(x.device),
           work={'family': 'norm', 'bytes': 3 * x2.numel() * 4})
    return y.view(x.shape)


def dropout_add_layernorm_backward(dy, x, r, gamma, eps, p, seed, need_x=True, need_r=True, need_params=True):
    d = x.shape[-1]
    dy2, x2, r2 = _rows(dy, d), _rows(x, d), _rows(r, d)
    rows = x2.shape[0]
    dx = torch.empty_like(x2) if need_x else None
    dr = torch.empty_like(x2) if need_r else None
    dg = torch.empty(d, dtype=torch.float32, device=x.device) if need_params else None
    db = torch.empty(d, dtype=torch.float32, device=x.device) if need_params else None
    ws = torch.empty(max(1, N.lib().kinet_dropout_add_layernorm_backward_workspace(rows, d)) if need_params else 1,
                     dtype=torch.float32, device=x.device)
    N.call('kinet_dropout_add_layernorm_backward', N.ptr(dy2), N.ptr(x2), N.ptr(r2), N.ptr(f32(gamma)), N.ptr(dx),
           N.ptr(dr), N.ptr(dg), N.ptr(db), rows, d, float(eps), float(p), N.ptr(seed), N.ptr(ws), N.stream(x.device),
           work={'family': 'norm', 'bytes': 5 * x2.numel() * 4})
    return (None if dx is None else dx.view(x.shape)), (None if dr is None else dr.view(x.shape)), dg, db


def dropout_act(x, p, seed, relu):
    """dropout_p(relu(x)) (relu optional), f32 (kinet_dropout_act)."""
    x = x.contiguous()
    y = torch.empty_like(x)
    N.call('kinet_dropout_act', N.ptr(x), N.ptr(y), x.numel(), int(relu), float(p), N.ptr(seed), N.stream(x.device),
           work={'family': 'eltwise', 'bytes': 2 * x.numel() * 4})
    return y


def dropout_act_backward(dy, y, p, seed, relu):
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    N.call('kinet_dropout_act_backward', N.ptr(dy), N.ptr(y), N.ptr(dx), dy.numel(), int(relu), float(p), N.ptr(seed),
           N.stream(dy.device), work={'family': 'eltwise', 'bytes': 3 * dy.numel() * 4})
    return dx


def _packed_rows(t):
    """(N, Lq, C) with unit column stride and packed batches -> its row stride (elements)."""
    if t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
        t = t.contiguous()
    return t, t.stride(1)


def msda_prep(offlog, refs, shapes, query_mask, heads, levels, points):
    """Sampling locations (N, Lq, M, L, P, 2) and attention weights (N, Lq, M, L, P) from the
    packed [sampling offsets | attention logits] projection (N, Lq, >= M*L*P*3)
    (ms_deform_attn.py:64-82), f32 (kinet_msda_prep)."""
    Nb, Lq = offlog.shape[:2]
    ol, ld = _packed_rows(offlog)
    rf = refs.contiguous()
    loc = torch.empty((Nb, Lq, heads, levels, points, 2), dtype=torch.float32, device=ol.device)
    attw = torch.empty((Nb, Lq, heads, levels, points), dtype=torch.float32, device=ol.device)
    qm = query_mask.to(torch.uint8).contiguous() if query_mask is not None else None
    N.call('kinet_msda_prep', N.ptr(ol), ld, N.ptr(rf), N.ptr(shapes.contiguous()), N.ptr(qm), N.ptr(loc),
           N.ptr(attw), Nb * Lq, heads, levels, points, rf.shape[-1], N.stream(ol.device),
           work={'family': 'msda_glue', 'bytes': 2 * (loc.numel() + attw.numel()) * 4})
    return loc, attw


def msda_prep_backward(grad_loc, grad_attw, attw, offlog, refs, shapes, heads, levels, points,
                       need_offlog=True, need_refs=True):
    """Gradients of msda_prep: w.r.t. the packed offlog (its layout, contiguous) and refs."""
    Nb, Lq = offlog.shape[:2]
    dev = offlog.device
    gl, ga = grad_loc.contiguous(), grad_attw.contiguous()
    ol = offlog.contiguous()      # the gradient takes offlog's (contiguous) layout
    ld = ol.shape[-1]
    rf = refs.contiguous()
    dol = torch.empty(ol.shape, dtype=torch.float32, device=dev) if need_offlog else None
    dref = torch.empty(rf.shape, dtype=torch.float32, device=dev) if need_refs else None
    N.call('kinet_msda_prep_backward', N.ptr(gl), N.ptr(ga), N.ptr(attw), N.ptr(ol), ld, N.ptr(rf),
           N.ptr(shapes.contiguous()), N.ptr(dol), N.ptr(dref), Nb * Lq, heads, levels, points, rf.shape[-1],
           N.stream(dev), work={'family': 'msda_glue', 'bytes': 3 * (gl.numel() + ga.numel()) * 4})
    return dol, dref


def inverse_sigmoid(x, eps=1e-5):
    x = x.contiguous()
    y = torch.empty_like(x)
    N.call('kinet_inverse_sigmoid', N.ptr(x), N.ptr(y), x.numel(), float(eps), N.stream(x.device),
           work={'family': 'eltwise', 'bytes': 2 * x.numel() * 4})
    return y


def inverse_sigmoid_backward(dy, x, eps=1e-5):
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    N.call('kinet_inverse_sigmoid_backward', N.ptr(dy), N.ptr(x), N.ptr(dx), dy.numel(), float(eps),
           N.stream(dy.device), work={'family': 'eltwise', 'bytes': 3 * dy.numel() * 4})
    return dx


def groupnorm_backward(dy, x, gamma, groups, eps, need_params=True):
    """x, dy (B, HW, C) NHWC."""
    B, HW, C = x.shape
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device) if need_params else None
    db = torch.empty(C, dtype=torch.float32, device=x.device) if need_params else None
    ws = torch.empty(max(1, N.lib().kinet_groupnorm_backward_workspace(B, HW, C, groups)), dtype=torch.float32,
                     device=x.device)
    N.call('kinet_groupnorm_backward', N.ptr(dy), N.ptr(x), N.ptr(f32(gamma)), N.ptr(dx), N.ptr(dg), N.ptr(db), B, HW,
           C, groups, float(eps), N.dtype_code(x.dtype), N.ptr(ws), N.stream(x.device),
           work={'family': 'norm', 'bytes': 4 * x.numel() * x.element_size()})
    return dx, dg, db


def mha_backward_qk(qk, v, do, heads, scale, key_mask=None, dropout_p=0.0, seed=None):
    """Backward of mha_core on the packed [q | k] projection qk (B, L, 2E) (self-attention,
    q = k input): returns dqk (B, L, 2E, the same packing -- the input gradient of ONE q|k
    projection GEMM) and dv."""
    B, L, E2 = qk.shape
    E = E2 // 2
    qk, v, do = qk.contiguous(), v.contiguous(), do.contiguous()
    for t in (qk, v, do):
        if t.dtype != torch.float32:
            raise RuntimeError('mha_backward_qk: f32 operands')
    dqk = torch.empty((B, L, E2), dtype=torch.float32, device=qk.device)
    dv = torch.empty((B, L, E), dtype=torch.float32, device=qk.device)
    ws = torch.empty(max(1, N.lib().kinet_mha_backward_workspace(B, L, L, heads)), dtype=torch.float32,
                     device=qk.device)
    km = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    N.call('kinet_mha_backward', N.ptr(qk), E2, N.ptr(qk[..., E:]), E2, N.ptr(v), E, N.ptr(do), E, N.ptr(dqk),
           N.ptr(dqk[..., E:]), N.ptr(dv), B, L, L, heads, E // heads, float(scale), N.ptr(km), N.ptr(ws),
           float(dropout_p), N.ptr(seed) if dropout_p > 0 else None, N.stream(qk.device),
           work={'family': 'attn', 'flops': 8.0 * B * heads * L * L * (E // heads)})
    return dqk, dv


def mha_backward(q, k, v, do, heads, scale, key_mask=None, dropout_p=0.0, seed=None):
    """Backward of mha_core (f32): returns dq, dk, dv with the layouts of q, k, v."""
    B, Lq, E = q.shape
    Lk = k.shape[1]
    for t in (q, k, v, do):
        if t.dtype != torch.float32 or t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise RuntimeError('mha_backward: f32 rows, unit stride, packed batches')
    dq = torch.empty((B, Lq, E), dtype=torch.float32, device=q.device)
    dk = torch.empty((B, Lk, E), dtype=torch.float32, device=q.device)
    dv = torch.empty((B, Lk, E), dtype=torch.float32, device=q.device)
    ws = torch.empty(max(1, N.lib().kinet_mha_backward_workspace(B, Lq, Lk, heads)), dtype=torch.float32,
                     device=q.device)
    km = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    # dq/dk/dv are written with q/k/v's row strides: give them packed copies of the layouts
    if q.stride(1) != E or k.stride(1) != E or v.stride(1) != E:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    N.call('kinet_mha_backward', N.ptr(q), E, N.ptr(k), E, N.ptr(v), E, N.ptr(do.contiguous()), E, N.ptr(dq),
           N.ptr(dk), N.ptr(dv), B, Lq, Lk, heads, E // heads, float(scale), N.ptr(km), N.ptr(ws), float(dropout_p),
           N.ptr(seed) if dropout_p > 0 else None, N.stream(q.device),
           work={'family': 'attn', 'flops': 8.0 * B * heads * Lq * Lk * (E // heads)})
    return dq, dk, dv


# field order of kinet_mha_train_plan's plan record (include/kinet_grad.h)
MHA_TRAIN_PLAN_FIELDS = ('supported', 'dense_default', 'qt', 'kt', 'row_stride', 'col_stride') + tuple(
    f'{k}_{f}' for k in ('fwd', 'dq', 'dkv') for f in ('grid_x', 'grid_y', 'grid_z', 'block', 'lds'))


def mha_train_plan(head_dim, batch, heads, Lq, Lk):
    """The launches of the f32 attention training pair for this problem (kinet_mha_train_plan,
    csrc/attn_train_plan.h; no GPU call): a dict of MHA_TRAIN_PLAN_FIELDS."""
    prob = (ctypes.c_int * 5)(head_dim, batch, heads, Lq, Lk)
    out = (ctypes.c_int * len(MHA_TRAIN_PLAN_FIELDS))()
    N.call('kinet_mha_train_plan', ctypes.cast(prob, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p))
    return dict(zip(MHA_TRAIN_PLAN_FIELDS, out))


def mha_train_calls():
    """kinet_mha_train_forward launches the calling thread has made so far."""
    return N.lib().kinet_mha_train_calls()


def _mha_train_rows(name, *ts):
    for t in ts:
        if t.dtype != torch.float32 or t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise RuntimeError(f'{name}: f32 rows, unit stride, packed batches')


def mha_train_forward(q, k, v, heads, scale, key_mask=None, dropout_p=0.0, seed=None, out=None):
    """mha_core for f32 training on the f32 MFMA (kinet_mha_train_forward; head_dim 32 / 36): returns
    o (B, Lq, E) and lse (B, heads, Lq), the log-sum-exp of the scaled scores over the unmasked keys."""
    B, Lq, E = q.shape
    Lk = k.shape[1]
    o = out if out is not None else torch.empty((B, Lq, E), dtype=torch.float32, device=q.device)
    _mha_train_rows('mha_train_forward', q, k, v, o)
    lse = torch.empty((B, heads, Lq), dtype=torch.float32, device=q.device)
    km = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    N.call('kinet_mha_train_forward', N.ptr(q), q.stride(1), N.ptr(k), k.stride(1), N.ptr(v), v.stride(1), N.ptr(o),
           o.stride(1), N.ptr(lse), B, Lq, Lk, heads, E // heads, float(scale), N.ptr(km), float(dropout_p),
           N.ptr(seed) if dropout_p > 0 else None, N.stream(q.device),
           work={'family': 'attn', 'flops': 4.0 * B * heads * Lq * Lk * (E // heads)})
    return o, lse


def mha_train_backward(q, k, v, o, do, lse, heads, scale, key_mask=None, dropout_p=0.0, seed=None, out=None):
    """Backward of mha_train_forward (kinet_mha_train_backward): dq, dk, dv with the row strides of q, k, v
    (`out`: the three tensors to write, laid out as q, k, v; default packed, for packed q, k, v)."""
    B, Lq, E = q.shape
    Lk = k.shape[1]
    if out is None:
        if q.stride(1) != E or k.stride(1) != E or v.stride(1) != E:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = tuple(torch.empty_like(t) for t in (q, k, v))
    dq, dk, dv = out
    _mha_train_rows('mha_train_backward', q, k, v, o, do, dq, dk, dv)
    if (dq.stride(1), dk.stride(1), dv.stride(1)) != (q.stride(1), k.stride(1), v.stride(1)):
        raise RuntimeError('mha_train_backward: dq / dk / dv take the row strides of q / k / v')
    ws = torch.empty(max(1, N.lib().kinet_mha_train_backward_workspace(B, Lq, heads)), dtype=torch.float32,
                     device=q.device)
    km = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    N.call('kinet_mha_train_backward', N.ptr(q), q.stride(1), N.ptr(k), k.stride(1), N.ptr(v), v.stride(1), N.ptr(o),
           o.stride(1), N.ptr(do), do.stride(1), N.ptr(lse.contiguous()), N.ptr(dq), N.ptr(dk), N.ptr(dv), B, Lq, Lk,
           heads, E // heads, float(scale), N.ptr(km), N.ptr(ws), float(dropout_p),
           N.ptr(seed) if dropout_p > 0 else None, N.stream(q.device),
           work={'family': 'attn', 'flops': 10.0 * B * heads * Lq * Lk * (E // heads)})
    return dq, dk, dv


# ------------------------------------------------------------------- segmentation head
def segm_attention(qp, kp, mask, Q, heads, out=None):
    """Joint-softmax attention map (kinet_segm_attention): qp (B*Q, d), kp (B, HW, d), mask (B, HW)
    bool / uint8 or None -> (B*Q, HW, heads) in qp's dtype, one softmax over heads x HW per row."""
    N.require_gpu(qp, kp)
    B, HW, d = kp.shape
    qp, kp = qp.contiguous(), kp.contiguous()
    if qp.shape != (B * Q, d) or kp.dtype != qp.dtype:
        raise RuntimeError(f'segm_attention: qp {tuple(qp.shape)} {qp.dtype} does not match kp {tuple(kp.shape)} {kp.dtype}')
    m = None
    if mask is not None:
        m = mask.reshape(B, HW).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)
    if out is None:
        out = torch.empty((B * Q, HW, heads), dtype=qp.dtype, device=qp.device)
    N.call('kinet_segm_attention', N.ptr(qp), N.ptr(kp), N.ptr(m), N.ptr(out), B, Q, HW, heads, d,
           float(d // heads) ** -0.5 if heads else 0.0, N.dtype_code(qp.dtype), N.stream(qp.device),
           work={'family': 'segm', 'flops': 4.0 * B * Q * HW * d})
    return out


def segm_lay1_weights(weight, d):
    """lay1's weight (Cout, d + Ca, 3, 3) split for the two parts of the convolution: the packed
    per-frame weights (Cout, 3, 3, d) per compute dtype come from pack_segm_lay1_src; this is the
    attention part as f32 (3, 3, Ca, Cout).  Cached per parameter version."""
    return cached(weight, ('segm_lay1_att', d),
                  lambda t: t.detach()[:, d:].permute(2, 3, 1, 0).float().contiguous())


def pack_segm_lay1_src(weight, d, dtype):
    """lay1's source-channel weights W[:, :d] packed OHWI in `dtype` (kinet_conv2d operand)."""
    return cached(weight, ('segm_lay1_src', d, dtype),
                  lambda t: t.detach()[:, :d].permute(0, 2, 3, 1).to(dtype).contiguous())


def _row_frame(row_frame, rows, what):
    """The ragged entry points' frame list: a contiguous device int32 tensor, one entry per row."""
    N.require_gpu(row_frame)
    if row_frame.dtype != torch.int32 or row_frame.dim() != 1 or row_frame.numel() != rows \
            or not row_frame.is_contiguous():
        raise RuntimeError(f'{what}: row_frame must be a contiguous int32 tensor of one frame per row ({rows}): got '
                           f'{row_frame.dtype} {tuple(row_frame.shape)}')
    return row_frame


def segm_attention_rows(qp, kp, mask, row_frame, heads, out=None):
    """segm_attention over gathered rows of several frames (kinet_segm_attention_rows): qp (rows, d), kp
    (B, HW, d), mask (B, HW) or None, row_frame (rows) device int32 -> (rows, HW, heads); row r attends
    frame row_frame[r], bit-identical to that row of segm_attention on its frame."""
    N.require_gpu(qp, kp)
    B, HW, d = kp.shape
    qp, kp = qp.contiguous(), kp.contiguous()
    rows = qp.shape[0]
    if qp.dim() != 2 or qp.shape[1] != d or kp.dtype != qp.dtype:
        raise RuntimeError(f'segm_attention_rows: qp {tuple(qp.shape)} {qp.dtype} does not match kp {tuple(kp.shape)} '
                           f'{kp.dtype}')
    _row_frame(row_frame, rows, 'segm_attention_rows')
    m = None
    if mask is not None:
        m = mask.reshape(B, HW).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)
    if out is None:
        out = torch.empty((rows, HW, heads), dtype=qp.dtype, device=qp.device)
    elif out.dtype != qp.dtype or tuple(out.shape) != (rows, HW, heads) or not out.is_contiguous():
        raise RuntimeError('segm_attention_rows: out must be contiguous (rows, HW, heads) in qp\'s dtype')
    N.call('kinet_segm_attention_rows', N.ptr(qp), N.ptr(kp), N.ptr(m), N.ptr(row_frame), N.ptr(out), rows, B, HW,
           heads, d, float(d // heads) ** -0.5 if heads else 0.0, N.dtype_code(qp.dtype), N.stream(qp.device),
           work={'family': 'segm', 'flops': 4.0 * rows * HW * d})
    return out


def segm_lay1(att, w_att, frame, row0, Q, row_frame=None, out=None):
    """y[r] = frame[(row0 + r) // Q] + conv3x3(att[r]; w_att) (kinet_segm_lay1): att (rows, H, W, 8),
    w_att (3, 3, 8, Cout) f32, frame (B, H, W, Cout) f32 -> (rows, H, W, Cout) in att's dtype.  With
    row_frame (rows, device int32) row r reads frame[row_frame[r]] instead (kinet_segm_lay1_rows; row0
    and Q are not used)."""
    N.require_gpu(att, frame)
    rows, H, W, Ca = att.shape
    B, Cout = frame.shape[0], frame.shape[3]
    if frame.dtype != torch.float32 or tuple(frame.shape[1:3]) != (H, W) or tuple(w_att.shape) != (3, 3, Ca, Cout):
        raise RuntimeError('segm_lay1: frame must be f32 (B, H, W, Cout) and w_att (3, 3, Ca, Cout)')
    if out is None:
        out = torch.empty((rows, H, W, Cout), dtype=att.dtype, device=att.device)
    elif out.dtype != att.dtype or tuple(out.shape) != (rows, H, W, Cout) or not out.is_contiguous():
        raise RuntimeError('segm_lay1: out must be contiguous (rows, H, W, Cout) in att\'s dtype')
    y = out
    work = {'family': 'segm', 'flops': 2.0 * rows * H * W * Cout * 9 * Ca, 'bytes': y.numel() * y.element_size()}
    if row_frame is not None:
        _row_frame(row_frame, rows, 'segm_lay1')
        N.call('kinet_segm_lay1_rows', N.ptr(att.contiguous()), N.ptr(w_att), N.ptr(frame.contiguous()),
               N.ptr(row_frame), N.ptr(y), rows, B, H, W, Ca, Cout, N.dtype_code(att.dtype), N.stream(att.device),
               work=work)
        return y
    N.call('kinet_segm_lay1', N.ptr(att.contiguous()), N.ptr(w_att), N.ptr(frame.contiguous()), N.ptr(y), rows, row0,
           Q, B, H, W, Ca, Cout, N.dtype_code(att.dtype), N.stream(att.device), work=work)
    return y


def segm_gn_relu(x, weight, bias, groups, eps=1e-5, fpn=None, row0=0, Q=None, row_frame=None, out=None):
    """relu(GroupNorm(x)) per row, optionally nearest-upsampled to fpn's size and added to
    fpn[(row0 + r) // Q] (kinet_segm_gn_relu_up_add): x (rows, h, w, C), fpn (B, H, W, C) or None.  With
    row_frame (rows, device int32) and an fpn, row r adds fpn[row_frame[r]] instead
    (kinet_segm_gn_relu_up_add_rows); without an fpn the list is not used."""
    N.require_gpu(x)
    rows, h, w, C = x.shape
    x = x.contiguous()
    if fpn is not None:
        if fpn.dtype != x.dtype or fpn.shape[3] != C:
            raise RuntimeError('segm_gn_relu: fpn must be (B, H, W, C) in x\'s dtype')
        fpn = fpn.contiguous()
        B, H, W = fpn.shape[:3]
    else:
        B, H, W, Q, row_frame = 1, h, w, None, None      # no per-frame operand: the rows are one "frame"
    Qn = int(Q) if Q is not None else max(rows + row0, 1)
    if out is None:
        out = torch.empty((rows, H, W, C), dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or tuple(out.shape) != (rows, H, W, C) or not out.is_contiguous():
        raise RuntimeError('segm_gn_relu: out must be contiguous (rows, H, W, C) in x\'s dtype')
    y = out
    ws = torch.empty(max(1, N.lib().kinet_segm_gn_workspace(rows, h * w, groups)), dtype=torch.float32, device=x.device)
    work = {'family': 'segm', 'bytes': (2 * x.numel() + y.numel()) * x.element_size()}
    if row_frame is not None:
        _row_frame(row_frame, rows, 'segm_gn_relu')
        N.call('kinet_segm_gn_relu_up_add_rows', N.ptr(x), N.ptr(f32(weight)), N.ptr(f32(bias)), N.ptr(fpn),
               N.ptr(row_frame), N.ptr(y), rows, B, h, w, H, W, C, groups, float(eps), N.dtype_code(x.dtype), N.ptr(ws),
               N.stream(x.device), work=work)
        return y
    N.call('kinet_segm_gn_relu_up_add', N.ptr(x), N.ptr(f32(weight)), N.ptr(f32(bias)), N.ptr(fpn), N.ptr(y), rows,
           row0, Qn, B, h, w, H, W, C, groups, float(eps), N.dtype_code(x.dtype), N.ptr(ws), N.stream(x.device),
           work=work)
    return y


def segm_out_weights(weight):
    """out_lay's weight (1, C, 3, 3) as f32 (3, 3, C), cached per parameter version."""
    return cached(weight, 'segm_out', lambda t: t.detach()[0].permute(1, 2, 0).float().contiguous())


def segm_out_conv(x, wt, bias, out=None):
    """3x3 pad-1 convolution to one channel (kinet_segm_out_conv): x (rows, H, W, C), wt (3, 3, C) f32,
    bias (1,) f32 -> (rows, H, W) f32."""
    N.require_gpu(x)
    rows, H, W, C = x.shape
    if out is None:
        out = torch.empty((rows, H, W), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * H * W:
        raise RuntimeError('segm_out_conv: out must be contiguous f32 (rows, H, W)')
    N.call('kinet_segm_out_conv', N.ptr(x.contiguous()), N.ptr(wt), N.ptr(bias), N.ptr(out), rows, H, W, C,
           N.dtype_code(x.dtype), N.stream(x.device),
           work={'family': 'segm', 'flops': 18.0 * rows * H * W * C, 'bytes': x.numel() * x.element_size()})
    return out


def segm_postprocess(logits, max_hw, img_hw, out_hw, threshold=0.5, return_probs=False):
    """PostProcessSegm for one frame (kinet_segm_postprocess): logits (Q, h, w) f32 -> (Q, 1, oh, ow)
    uint8 (probability > threshold) or f32 probabilities.  Sizes are host ints."""
    N.require_gpu(logits)
    logits = logits.float().contiguous()
    Q, h, w = logits.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((Q, 1, oh, ow), dtype=torch.float32 if return_probs else torch.uint8, device=logits.device)
    N.call('kinet_segm_postprocess', N.ptr(logits), N.ptr(out), Q, h, w, int(max_hw[0]), int(max_hw[1]),
           int(img_hw[0]), int(img_hw[1]), oh, ow, float(threshold), int(return_probs), N.stream(logits.device),
           work={'family': 'segm', 'bytes': out.numel() * out.element_size()})
    return out


def segm_track_resolve(logits, src, prev_labels, max_hw, img_hw, out_hw, threshold=0.5, out=None):
    """The tracker's overlap resolution for one frame (kinet_segm_track_resolve): logits (n, h, w) f32
    fresh mask logits, `src` a HOST sequence of T ints (>= 0: a row of logits, < 0: slot -s-1 of
    prev_labels), prev_labels (oh, ow) int16 or None -> (oh, ow) int16 labels, -1 = background,
    labels == t the exclusive mask of slot t.  `src` may also be a device int32 tensor (not checked)."""
    N.require_gpu(logits, prev_labels, out)
    logits = logits.float().contiguous()
    n, h, w = logits.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if torch.is_tensor(src):
        if src.dtype != torch.int32 or not src.is_cuda:
            raise RuntimeError('segm_track_resolve: a tensor src must be int32 on the GPU')
        src_dev, T = src.contiguous(), src.numel()
    else:
        src = [int(s) for s in src]
        T = len(src)
        if any(s >= n for s in src):
            raise RuntimeError(f'segm_track_resolve: a fresh slot names a row outside the {n} rows of logits')
        if any(s < 0 for s in src):
            if prev_labels is None:
                raise RuntimeError('segm_track_resolve: a stale slot needs prev_labels')
            if any(-s - 1 > 32767 for s in src):
                raise RuntimeError('segm_track_resolve: a stale slot names a slot beyond int16')
        src_dev = torch.tensor(src, dtype=torch.int32, device=logits.device) if T else None
    if prev_labels is not None and (prev_labels.dtype != torch.int16 or tuple(prev_labels.shape) != (oh, ow)
                                    or not prev_labels.is_contiguous()):
        raise RuntimeError('segm_track_resolve: prev_labels must be contiguous int16 (oh, ow)')
    if out is None:
        out = torch.empty((oh, ow), dtype=torch.int16, device=logits.device)
    elif out.dtype != torch.int16 or tuple(out.shape) != (oh, ow) or not out.is_contiguous():
        raise RuntimeError('segm_track_resolve: out must be contiguous int16 (oh, ow)')
    N.call('kinet_segm_track_resolve', N.ptr(logits) if n else None, N.ptr(src_dev), N.ptr(prev_labels), N.ptr(out),
           T, n, h, w, int(max_hw[0]), int(max_hw[1]), int(img_hw[0]), int(img_hw[1]), oh, ow, float(threshold),
           N.stream(logits.device), work={'family': 'segm', 'bytes': out.numel() * 4})
    return out


RESOLVE_STAT_BYTES = 20     # (count, x0, y0, x1, y1) int32 per slot of kinet_segm_track_resolve_segments


def segm_resolve_views(buf, total, pixels):
    """(stats (total, 5) int32, labels (pixels,) int16) of a packed kinet_segm_track_resolve_segments buffer
    (a uint8 torch tensor or numpy array: stats first, then the sequences' label maps)."""
    nb = RESOLVE_STAT_BYTES * total
    if isinstance(buf, torch.Tensor):
        return buf[:nb].view(torch.int32).view(total, 5), buf[nb:nb + 2 * pixels].view(torch.int16)
    import numpy as np
    return buf[:nb].view(np.int32).reshape(total, 5), buf[nb:nb + 2 * pixels].view(np.int16)


def segm_track_resolve_segments(logits, src, src_off, geom, prev_labels, prev_off, max_hw, threshold=0.5, out=None):
    """The tracker's overlap resolution for S sequences in one launch (kinet_segm_track_resolve_segments).
    logits (n, h, w) f32: the kept rows of all sequences; src: DEVICE int32 (total), sequence s's slots
    src[src_off[s]:src_off[s + 1]] (>= 0: a row of logits, < 0: slot -e-1 of its previous map); src_off a HOST
    sequence of S + 1 ints; geom a HOST (S, 4) of (img_h, img_w, oh, ow), oh*ow == 0 for a sequence without a
    map; prev_labels: the previous call's labels view (device int16) or None; prev_off a HOST sequence of S
    element offsets into it, < 0 (or None) for no previous map.
    -> (buf, stats, labels, pix_off): buf one uint8 allocation (stats | labels, a multiple of 4 bytes: one
    copy carries both), stats (total, 5) int32 = (count, x0, y0, x1, y1) per slot, labels int16 (pixels,) with
    sequence s's (oh, ow) map at pix_off[s]:pix_off[s + 1] holding LOCAL slot indices or -1.  `out`: a uint8
    device buffer to reuse when it is large enough (it must not hold prev_labels)."""
    import numpy as np
    N.require_gpu(logits, src, prev_labels, out)
    logits = logits.float().contiguous()
    n, h, w = logits.shape
    src_off = np.ascontiguousarray(np.asarray(src_off, np.int64).reshape(-1))
    S = src_off.size - 1
    geom = np.ascontiguousarray(np.asarray(geom, np.int64).reshape(-1, 4))
    if S < 0 or geom.shape[0] != S:
        raise RuntimeError('segm_track_resolve_segments: src_off (S + 1) and geom (S, 4)')
    if S and (src_off[0] != 0 or (np.diff(src_off) < 0).any()):
        raise RuntimeError('segm_track_resolve_segments: src_off must start at 0 and ascend')
    if S and (np.diff(src_off) > 32767).any():
        raise RuntimeError('segm_track_resolve_segments: a segment holds at most 32767 slots (labels are int16)')
    total = int(src_off[-1]) if S else 0
    if (geom < 0).any() or (geom > 0x7fffffff).any():
        raise RuntimeError('segm_track_resolve_segments: geom out of range')
    px = geom[:, 2] * geom[:, 3]
    live = px > 0
    if (live & ((geom[:, 0] < 1) | (geom[:, 0] > int(max_hw[0])) | (geom[:, 1] < 1) | (geom[:, 1] > int(max_hw[1])))).any():
        raise RuntimeError('segm_track_resolve_segments: a frame\'s size must lie inside max_hw')
    if total:
        if src is None or src.dtype != torch.int32 or src.numel() != total or not src.is_contiguous():
            raise RuntimeError(f'segm_track_resolve_segments: src must be a contiguous device int32 tensor of {total} slots')
    pix_off = np.zeros(S + 1, np.int64)
    pix_off[1:] = np.cumsum(px)
    pixels = int(pix_off[-1])
    poff = np.full(S, -1, np.int64) if prev_off is None else np.ascontiguousarray(np.asarray(prev_off, np.int64).reshape(-1))
    if poff.size != S:
        raise RuntimeError('segm_track_resolve_segments: prev_off holds one offset per sequence')
    poff = np.where(live, poff, -1)
    if (poff >= 0).any():
        if prev_labels is None or prev_labels.dtype != torch.int16 or not prev_labels.is_contiguous():
            raise RuntimeError('segm_track_resolve_segments: a previous map needs prev_labels, contiguous int16')
        if (poff + px > prev_labels.numel())[poff >= 0].any():
            raise RuntimeError('segm_track_resolve_segments: a previous map reaches beyond prev_labels')
    nbytes = (RESOLVE_STAT_BYTES * total + 2 * pixels + 3) // 4 * 4
    if out is None or out.numel() < nbytes:
        out = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=logits.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.data_ptr() % 4:
        raise RuntimeError('segm_track_resolve_segments: out must be a contiguous, 4-byte aligned uint8 buffer')
    buf = out[:nbytes]
    stats, labels = segm_resolve_views(buf, total, pixels)
    if not total and not pixels:
        return buf, stats, labels, pix_off
    if prev_labels is not None and pixels:
        lo, hi = labels.data_ptr(), labels.data_ptr() + 2 * pixels
        plo, phi = prev_labels.data_ptr(), prev_labels.data_ptr() + 2 * prev_labels.numel()
        if lo < phi and plo < hi:
            raise RuntimeError('segm_track_resolve_segments: out and prev_labels must be two buffers')
    so, ge = src_off.astype(np.int32), geom.astype(np.int32)
    N.call('kinet_segm_track_resolve_segments', N.ptr(logits) if n else None, N.ptr(src) if total else None,
           so.ctypes.data, ge.ctypes.data, pix_off.ctypes.data, N.ptr(prev_labels) if (poff >= 0).any() else None,
           poff.ctypes.data, N.ptr(labels) if pixels else None, N.ptr(stats) if total else None, S, total, n, h, w,
           int(max_hw[0]), int(max_hw[1]), float(threshold), N.stream(logits.device),
           work={'family': 'segm', 'bytes': pixels * 4 + total * RESOLVE_STAT_BYTES})
    return buf, stats, labels, pix_off


# ------------------------------------------------------------------- mask training
MASK_LOSS_ALPHA, MASK_LOSS_GAMMA = 0.25, 2.0     # detr.py:788 calls sigmoid_focal_loss with its defaults


def _ws(n, device):
    return torch.empty(max(1, int(n)), dtype=torch.float32, device=device)


def _mask_loss_args(logits, target):
    N.require_gpu(logits, target)
    if logits.dtype != torch.float32 or logits.dim() != 3 or target.dtype != torch.uint8 or target.dim() != 3 \
            or target.shape[0] != logits.shape[0]:
        raise RuntimeError(f'segm_mask_loss: logits must be f32 (n, h, w) and target uint8 (n, H, W): got '
                           f'{tuple(logits.shape)} {logits.dtype}, {tuple(target.shape)} {target.dtype}')
    return logits.contiguous(), target.contiguous()


def segm_mask_loss(logits, target, num_boxes, alpha=MASK_LOSS_ALPHA, gamma=MASK_LOSS_GAMMA):
    """The fused mask losses (kinet_segm_mask_loss): logits (n, h, w) f32, target (n, H, W) uint8 0/1 ->
    (loss (2,) f32 = [focal, dice], sums (n, 4) f32 per-row [focal, p*t, p, t] sums the backward reads)."""
    logits, target = _mask_loss_args(logits, target)
    n, h, w = logits.shape
    H, W = target.shape[1:]
    loss = torch.empty(2, dtype=torch.float32, device=logits.device)
    sums = torch.empty((n, 4), dtype=torch.float32, device=logits.device)
    ws = _ws(N.lib().kinet_segm_mask_loss_workspace(n, H, W), logits.device)
    N.call('kinet_segm_mask_loss', N.ptr(logits), N.ptr(target), N.ptr(sums), N.ptr(loss), n, h, w, H, W, float(alpha),
           float(gamma), float(num_boxes), N.ptr(ws), N.stream(logits.device),
           work={'family': 'segm_loss', 'bytes': target.numel() + 4 * logits.numel()})
    return loss, sums


def segm_mask_loss_backward(logits, target, sums, dloss, num_boxes, alpha=MASK_LOSS_ALPHA, gamma=MASK_LOSS_GAMMA):
    """d(dloss . loss) / dlogits of segm_mask_loss (kinet_segm_mask_loss_backward): dloss (2,) f32 on the
    device -> (n, h, w) f32."""
    logits, target = _mask_loss_args(logits, target)
    N.require_gpu(sums, dloss)
    n, h, w = logits.shape
    H, W = target.shape[1:]
    if sums.dtype != torch.float32 or tuple(sums.shape) != (n, 4) or dloss.dtype != torch.float32 or dloss.numel() != 2:
        raise RuntimeError('segm_mask_loss_backward: sums must be f32 (n, 4) and dloss f32 (2,)')
    dlogits = torch.empty_like(logits)
    N.call('kinet_segm_mask_loss_backward', N.ptr(logits), N.ptr(target), N.ptr(sums.contiguous()),
           N.ptr(dloss.contiguous()), N.ptr(dlogits), n, h, w, H, W, float(alpha), float(gamma), float(num_boxes),
           N.stream(logits.device), work={'family': 'segm_loss', 'bytes': target.numel() + 8 * logits.numel()})
    return dlogits


def segm_attention_backward(datt, att, qp, kp, Q, heads, need_q=True, need_k=True):
    """Backward of segm_attention in f32 (kinet_segm_attention_backward): datt, att (B*Q, HW, heads),
    qp (B*Q, d), kp (B, HW, d) -> (dqp, dkp), None where not needed."""
    N.require_gpu(datt, att, qp, kp)
    B, HW, d = kp.shape
    datt, att, qp, kp = datt.contiguous(), att.contiguous(), qp.contiguous(), kp.contiguous()
    if any(t.dtype != torch.float32 for t in (datt, att, qp, kp)) or qp.shape != (B * Q, d) \
            or att.shape != (B * Q, HW, heads) or datt.shape != att.shape:
        raise RuntimeError('segm_attention_backward: f32 datt / att (B*Q, HW, heads), qp (B*Q, d), kp (B, HW, d)')
    dqp = torch.empty_like(qp) if need_q else None
    dkp = torch.empty_like(kp) if need_k else None
    ws = _ws(N.lib().kinet_segm_attention_backward_workspace(B, Q), qp.device)
    N.call('kinet_segm_attention_backward', N.ptr(datt), N.ptr(att), N.ptr(qp), N.ptr(kp), N.ptr(dqp), N.ptr(dkp), B, Q,
           HW, heads, d, float(d // heads) ** -0.5, N.ptr(ws), N.stream(qp.device),
           work={'family': 'segm', 'flops': 8.0 * B * Q * HW * d})
    return dqp, dkp


def _relu_up_add_geometry(x, f, row0, Q, size):
    rows, h, w, C = x.shape
    if f is not None:
        if f.dtype != torch.float32 or f.dim() != 4 or f.shape[3] != C:
            raise RuntimeError('segm_relu_up_add: f must be f32 (B, H, W, C)')
        B, H, W = f.shape[:3]
    else:
        B, (H, W) = 1, ((h, w) if size is None else size)
        Q = None
    return rows, h, w, C, B, int(H), int(W), int(Q) if Q is not None else max(rows + row0, 1)


def segm_relu_up_add(x, f=None, row0=0, Q=None, size=None):
    """y = f[(row0 + r) // Q] + nearest-upsampled relu(x) in f32 (kinet_segm_relu_up_add): x (rows, h, w, C),
    f (B, H, W, C) or None (the output then has x's size)."""
    N.require_gpu(x, f)
    if x.dtype != torch.float32:
        raise RuntimeError('segm_relu_up_add: f32 only (the training path)')
    x = x.contiguous()
    f = None if f is None else f.contiguous()
    rows, h, w, C, B, H, W, Qn = _relu_up_add_geometry(x, f, row0, Q, size)
    y = torch.empty((rows, H, W, C), dtype=torch.float32, device=x.device)
    N.call('kinet_segm_relu_up_add', N.ptr(x), N.ptr(f), N.ptr(y), rows, row0, Qn, B, h, w, H, W, C, N.stream(x.device),
           work={'family': 'segm', 'bytes': 4 * (x.numel() + 2 * y.numel())})
    return y


def segm_relu_up_add_backward(dy, x, f_shape=None, row0=0, Q=None, need_x=True, need_f=True):
    """Backward of segm_relu_up_add (kinet_segm_relu_up_add_backward): dy (rows, H, W, C), x (rows, h, w, C),
    f_shape the FPN operand's (B, H, W, C) or None -> (dx, df), None where not needed.  df sums this
    call's rows only."""
    N.require_gpu(dy, x)
    dy, x = dy.contiguous(), x.contiguous()
    rows, h, w, C = x.shape
    H, W = dy.shape[1:3]
    if dy.dtype != torch.float32 or x.dtype != torch.float32 or dy.shape[0] != rows or dy.shape[3] != C:
        raise RuntimeError('segm_relu_up_add_backward: f32 dy (rows, H, W, C) and x (rows, h, w, C)')
    if f_shape is None:
        B, Qn, need_f = 1, max(rows + row0, 1), False
    else:
        if tuple(f_shape[1:]) != (H, W, C):
            raise RuntimeError('segm_relu_up_add_backward: f_shape must be (B, H, W, C) of dy')
        B, Qn = int(f_shape[0]), int(Q) if Q is not None else max(rows + row0, 1)
    dx = torch.empty_like(x) if need_x else None
    df = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device) if need_f else None
    N.call('kinet_segm_relu_up_add_backward', N.ptr(dy), N.ptr(x), N.ptr(dx), N.ptr(df), rows, row0, Qn, B, h, w, H, W, C,
           N.stream(x.device), work={'family': 'segm', 'bytes': 4 * (2 * dy.numel() + 2 * x.numel())})
    return dx, df


def segm_out_conv_backward(dy, x, wt, need_x=True, need_w=True):
    """Backward of segm_out_conv in f32 (kinet_segm_out_conv_backward): dy (rows, H, W), x (rows, H, W, C),
    wt (3, 3, C) -> (dx, dwt (3, 3, C), dbias (1,)), None where not needed."""
    N.require_gpu(dy, x, wt)
    dy, x, wt = dy.contiguous(), x.contiguous(), wt.contiguous()
    rows, H, W, C = x.shape
    if any(t.dtype != torch.float32 for t in (dy, x, wt)) or tuple(dy.shape) != (rows, H, W) or tuple(wt.shape) != (3, 3, C):
        raise RuntimeError('segm_out_conv_backward: f32 dy (rows, H, W), x (rows, H, W, C), wt (3, 3, C)')
    dx = torch.empty_like(x) if need_x else None
    dwt = torch.empty_like(wt) if need_w else None
    db = torch.empty(1, dtype=torch.float32, device=x.device) if need_w else None
    ws = _ws(N.lib().kinet_segm_out_conv_backward_workspace(rows, H, W, C), x.device) if need_w else None
    N.call('kinet_segm_out_conv_backward', N.ptr(dy), N.ptr(x), N.ptr(wt), N.ptr(dx), N.ptr(dwt), N.ptr(db), rows, H, W,
           C, N.ptr(ws), N.stream(x.device), work={'family': 'segm', 'bytes': 4 * (dy.numel() + 2 * x.numel())})
    return dx, dwt, db


# ------------------------------------------------------------------- multi-sequence tracker
TRACK_MAX_ROWS = 4096                       # KINET_TRACK_MAX_ROWS (include/kinet_track.h)
TRACK_DEC_TRACK, TRACK_DEC_REID, TRACK_DEC_DET, TRACK_DEC_PERSON = 1, 2, 4, 8


def _track_arg(t, dtype, what):
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f'{what} must be contiguous {dtype}: got {t.dtype}, strides {t.stride()}')
    return t


def track_decide_views(out, S, N_):
    """(boxes (S, N, 4) f32, scores (S, N) f32, labels (S, N) int32, decisions (S, N) uint8) of a packed
    kinet_track_decide buffer (a uint8 torch tensor or numpy array of S*N*25 bytes)."""
    r = S * N_
    if isinstance(out, torch.Tensor):
        return (out[:16 * r].view(torch.float32).view(S, N_, 4), out[16 * r:20 * r].view(torch.float32).view(S, N_),
                out[20 * r:24 * r].view(torch.int32).view(S, N_), out[24 * r:25 * r].view(S, N_))
    import numpy as np
    return (out[:16 * r].view(np.float32).reshape(S, N_, 4), out[16 * r:20 * r].view(np.float32).reshape(S, N_),
            out[20 * r:24 * r].view(np.int32).reshape(S, N_), out[24 * r:25 * r].reshape(S, N_))


def track_decide(pred_logits, pred_boxes, sizes, n_active, n_inactive, Kmax, track_thresh, reid_thresh,
                 detection_thresh, clip, out=None):
    """DeformablePostProcess + clip_boxes_to_image + the tracker's threshold compares for S sequences in
    one launch (kinet_track_decide): pred_logits (S, N, C) f32, pred_boxes (S, N, 4) f32, sizes (S, 2) f32
    (h, w), n_active / n_inactive (S) int32 -> one packed uint8 buffer (S*N*25 bytes; track_decide_views)."""
    N.require_gpu(pred_logits, pred_boxes, sizes, n_active, n_inactive, out)
    if pred_logits.dim() != 3 or pred_boxes.shape != pred_logits.shape[:2] + (4,):
        raise RuntimeError(f'track_decide: pred_logits (S, N, C) and pred_boxes (S, N, 4): got '
                           f'{tuple(pred_logits.shape)}, {tuple(pred_boxes.shape)}')
    S, N_, C = pred_logits.shape
    _track_arg(pred_logits, torch.float32, 'track_decide: pred_logits')
    _track_arg(pred_boxes, torch.float32, 'track_decide: pred_boxes')
    _track_arg(sizes, torch.float32, 'track_decide: sizes')
    _track_arg(n_active, torch.int32, 'track_decide: n_active')
    _track_arg(n_inactive, torch.int32, 'track_decide: n_inactive')
    if tuple(sizes.shape) != (S, 2) or n_active.numel() != S or n_inactive.numel() != S:
        raise RuntimeError('track_decide: sizes must be (S, 2) and the counts (S,)')
    if out is None:
        out = torch.empty(S * N_ * 25, dtype=torch.uint8, device=pred_logits.device)
    elif out.dtype != torch.uint8 or out.numel() != S * N_ * 25 or not out.is_contiguous():
        raise RuntimeError('track_decide: out must be a contiguous uint8 buffer of S*N*25 bytes')
    N.call('kinet_track_decide', N.ptr(pred_logits), N.ptr(pred_boxes), N.ptr(sizes), N.ptr(n_active), N.ptr(n_inactive),
           N.ptr(out), S, N_, C, int(Kmax), float(track_thresh), float(reid_thresh), float(detection_thresh),
           1 if clip else 0, N.stream(pred_logits.device), work={'family': 'track', 'bytes': S * N_ * (4 * C + 41)})
    return out


def nms_segments(boxes, scores, idx, offsets, total, iou_threshold, inf_flag=None, keep=None):
    """S independent NMS problems in one launch (kinet_nms_segments): boxes (rows, 4) and scores (rows) f32
    views of a shared bank (any row stride, unit inner stride), idx (>= total) int32 bank rows, offsets
    (S + 1) int32, inf_flag (>= total) uint8 or None -> keep (total) uint8, one byte per list entry."""
    N.require_gpu(boxes, scores, idx, offsets, inf_flag, keep)
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4 \
            or scores.dim() != 1 or scores.shape[0] != boxes.shape[0] or (boxes.shape[0] and boxes.stride(1) != 1):
        raise RuntimeError('nms_segments: boxes (rows, 4) with unit inner stride and scores (rows) in f32')
    _track_arg(idx, torch.int32, 'nms_segments: idx')
    _track_arg(offsets, torch.int32, 'nms_segments: offsets')
    S, total = offsets.numel() - 1, int(total)
    if S < 0 or idx.numel() < total or (inf_flag is not None and (inf_flag.dtype != torch.uint8 or inf_flag.numel() < total
                                                                    or not inf_flag.is_contiguous())):
        raise RuntimeError('nms_segments: offsets (S + 1), idx and inf_flag (uint8) of at least `total` entries')
    if keep is None:
        keep = torch.empty(total, dtype=torch.uint8, device=boxes.device)
    elif keep.dtype != torch.uint8 or keep.numel() < total or not keep.is_contiguous():
        raise RuntimeError('nms_segments: keep must be contiguous uint8 of at least `total` entries')
    rows = boxes.shape[0]
    N.call('kinet_nms_segments', N.ptr(boxes), max(boxes.stride(0), 4) if rows else 4, N.ptr(scores),
           max(scores.stride(0), 1) if rows else 1, rows, N.ptr(idx), N.ptr(offsets), N.ptr(inf_flag), N.ptr(keep), S,
           total, float(iou_threshold), N.stream(boxes.device), work={'family': 'track', 'bytes': 24 * total})
    return keep


def track_commit(hs_embed, boxes, scores, rows, slots, n, bank):
    """bank[slots[p]] = (hs_embed[rows[p]] | boxes[rows[p]] | scores[rows[p]]), p < n (kinet_track_commit):
    hs_embed (R, d), boxes (R, 4), scores (R) f32 of the frame, rows / slots int32 (>= n), bank (capacity, d + 5)."""
    N.require_gpu(hs_embed, boxes, scores, rows, slots, bank)
    R, d = hs_embed.shape
    for t, what in ((hs_embed, 'hs_embed'), (boxes, 'boxes'), (scores, 'scores'), (bank, 'bank')):
        _track_arg(t, torch.float32, 'track_commit: ' + what)
    _track_arg(rows, torch.int32, 'track_commit: rows')
    _track_arg(slots, torch.int32, 'track_commit: slots')
    if boxes.numel() != 4 * R or scores.numel() != R or bank.dim() != 2 or bank.shape[1] != d + 5 \
            or rows.numel() < n or slots.numel() < n:
        raise RuntimeError('track_commit: boxes (R, 4), scores (R), bank (capacity, d + 5), n rows and slots')
    N.call('kinet_track_commit', N.ptr(hs_embed), N.ptr(boxes), N.ptr(scores), R, N.ptr(rows), N.ptr(slots), int(n),
           N.ptr(bank), bank.shape[0], d, N.stream(bank.device), work={'family': 'track', 'bytes': 8 * n * (d + 5)})


def track_gather(bank, slots, offsets, sizes, Kmax, Q):
    """Next frame's track queries (kinet_track_gather): bank (capacity, d + 5) f32, slots int32, offsets
    (S + 1) int32, sizes (S, 2) f32 (h, w) -> (embeds (S, Kmax, d) f32, cxcywh boxes (S, Kmax, 4) f32
    normalised by the frame size, placeholder mask (S, Kmax + Q) bool)."""
    N.require_gpu(bank, slots, offsets, sizes)
    _track_arg(bank, torch.float32, 'track_gather: bank')
    _track_arg(slots, torch.int32, 'track_gather: slots')
    _track_arg(offsets, torch.int32, 'track_gather: offsets')
    _track_arg(sizes, torch.float32, 'track_gather: sizes')
    S, d = offsets.numel() - 1, bank.shape[1] - 5
    if bank.dim() != 2 or d < 1 or tuple(sizes.shape) != (S, 2):
        raise RuntimeError('track_gather: bank (capacity, d + 5), offsets (S + 1), sizes (S, 2)')
    dev = bank.device
    embeds = torch.empty((S, Kmax, d), dtype=torch.float32, device=dev)
    boxes = torch.empty((S, Kmax, 4), dtype=torch.float32, device=dev)
    mask = torch.empty((S, Kmax + Q), dtype=torch.bool, device=dev)
    N.call('kinet_track_gather', N.ptr(bank), bank.shape[0], d, N.ptr(slots), N.ptr(offsets), N.ptr(sizes), N.ptr(embeds),
           N.ptr(boxes), N.ptr(mask), S, int(Kmax), int(Q), N.stream(dev),
           work={'family': 'track', 'bytes': 8 * S * Kmax * (d + 4)})
    return embeds, boxes, mask


def track_reid_dist(bank, hs_embed, slots, slot_off, rows, row_off, out_off, total):
    """||bank_embed - hs_embed + 1e-6||_2 for every (inactive slot, detection row) pair of every sequence
    (kinet_track_reid_dist), packed: sequence s's (a, b) matrix at out[out_off[s]:out_off[s + 1]]."""
    N.require_gpu(bank, hs_embed, slots, slot_off, rows, row_off, out_off)
    _track_arg(bank, torch.float32, 'track_reid_dist: bank')
    _track_arg(hs_embed, torch.float32, 'track_reid_dist: hs_embed')
    for t in (slots, slot_off, rows, row_off, out_off):
        _track_arg(t, torch.int32, 'track_reid_dist: index lists')
    R, d = hs_embed.shape
    S = out_off.numel() - 1
    if bank.dim() != 2 or bank.shape[1] != d + 5 or slot_off.numel() != S + 1 or row_off.numel() != S + 1:
        raise RuntimeError('track_reid_dist: bank (capacity, d + 5), hs_embed (R, d), three (S + 1) offset lists')
    out = torch.empty(int(total), dtype=torch.float32, device=bank.device)
    N.call('kinet_track_reid_dist', N.ptr(bank), bank.shape[0], N.ptr(hs_embed), R, d, N.ptr(slots), N.ptr(slot_off),
           N.ptr(rows), N.ptr(row_off), N.ptr(out_off), N.ptr(out), S, int(total), N.stream(bank.device),
           work={'family': 'track', 'bytes': 8 * int(total) * d})
    return out
