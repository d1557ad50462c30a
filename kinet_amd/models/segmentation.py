"""Segmentation heads of Deformable DETR on the kinet_amd kernels.

Mirrors src/trackformer/models/detr_segmentation.py: DETRSegmBase :29-71, DeformableDETRSegm
:81-84, DeformableDETRSegmTracking :94-98, MaskHeadSmallConv :105-178, MHAttentionMap :181-216 and
PostProcessSegm :219-253, with identical module / parameter names (`bbox_attention.{q,k}_linear`,
`mask_head.{lay1..5, gn1..5, out_lay, adapter1..3}`), MRO and constructor arguments, so the
reference's checkpoints load unchanged.  `out['pred_masks']` is f32 (B, Q_total, H/4, W/4) and the
fourth return value is the memory LEVEL (B, d, h, w) the attention map reads, not the list.

The head runs csrc/segm.hip (include/kinet_segm.h) and kinet_conv2d in the compute dtype:
  * attention map: q_linear / k_linear are GEMMs on rows, then one joint softmax over heads x h*w;
  * lay1 (d+8 -> d+8, 3x3) is linear in its concatenated input [src | attention], so its src part
    (+ bias) is ONE f32 convolution per frame and only the 8 attention channels (K = 72) are
    convolved per query, added to the frame part broadcast over the frame's queries;
  * GroupNorm + ReLU (+ nearest upsample + FPN add) is one entry point; lay2..lay5 are
    kinet_conv2d; out_lay (16 -> 1) is a direct kernel; the adapters are 1x1 GEMMs once per frame.
Rows are frame-major (row b*Q + q, `_expand` of :101-102).  The head runs over chunks of rows
(`mask_query_chunk`, None = sized to `MASK_WORKSPACE_BYTES`); nothing reduces across rows and no
kernel choice depends on the chunk (split-K is off), so pred_masks does not depend on the chunking.

`defer_masks` (the tracker's MOTS path): forward returns `out` without 'pred_masks' and keeps the
head's operands until the next forward; `mask_logits(rows, frame)` then runs the attention map and
the head on the chosen query rows only, bit-identical to those rows of the full head;
`mask_logits_rows(rows, frames)` does so for rows of several frames in ONE pass (the multi-sequence
tracker's path): the kernels that read a per-frame operand take the rows' frames as a device list.

Mask training (opt-in: `mask_training = True`, set by kinet_amd.train.build_mask_training; a model
from build_model raises under autograd as before).  Off the fast path the detector runs
_forward_reference (for the tracking class the two-pass forward; the head reads the last,
current-frame pass) and `pred_masks` comes from ONE autograd Function over (hs[-1], the memory
level's rows, the level-1 input projection, the three FPN features, the head's parameters):
  * forward: the inference head above, in f32, over all B*Q rows in chunks, nothing kept but the inputs;
  * backward: loss_masks reads the matcher's matched rows only, mask losses are skipped for the aux
    outputs and rows never mix (GroupNorm statistics are per row), so the gradient of an unmatched
    row is exactly zero: the rows whose incoming gradient is not all zero are found (ONE host sync
    per step, next to the matcher's), and per frame the differentiable head -- kinet_amd.autograd
    Functions only: linear, segm_attention, conv_nhwc (lay1 as its frame part and its 8-channel
    part through weight slices), group_norm_nhwc, segm_relu_up_add, segm_out_conv -- is recomputed
    on those rows alone and back-propagated.  Differentiating all B*Q rows would materialise
    im2col for every row (about 40 GB for lay5 at 600 rows of 200 x 334).
So the loss VALUE comes from the inference kernels' logits and the GRADIENT from the recomputed
activations: two f32 evaluations of the same function whose roundings differ (fused GroupNorm vs
its own Function, the convolutions' epilogues).  tests/test_segm_train_gpu.py holds both to the
reference's losses and gradients.

Not built (NotImplementedError): vanilla DETRSegm, masks with two_stage, PostProcessPanoptic.
Reference defect: DETRSegmBase.forward(samples, targets) drops `prev_features`, so the reference
tracker's three-argument call (tracker.py:309) is a TypeError with a masks model; here
forward(samples, targets=None, prev_features=None) passes it on.
"""
import torch
from torch import nn

from kinet_amd import autograd as A
from kinet_amd import kernels as K
from kinet_amd.models.deformable_detr import DeformableDETR
from kinet_amd.models.deformable_transformer import fast_path
from kinet_amd.models.detr_tracking import DETRTrackingBase

MASK_WORKSPACE_BYTES = 256 << 20   # bound on one chunk's largest pair of activations


class MHAttentionMap(nn.Module):
    """detr_segmentation.py:181-216: the attention softmax alone (no product with values), ONE
    softmax over heads x pixels.  forward works on rows: q (B*Q, d), k (B, h*w, d)."""

    def __init__(self, query_dim, hidden_dim, num_heads, dropout=0.0, bias=True):
        super().__init__()
        if dropout:
            raise NotImplementedError('MHAttentionMap: the reference builds it with dropout 0.0')
        self.num_heads = num_heads
        self.hidden_dim = hidden_dim
        self.dropout = nn.Dropout(dropout)
        self.q_linear = nn.Linear(query_dim, hidden_dim, bias=bias)
        self.k_linear = nn.Linear(query_dim, hidden_dim, bias=bias)
        nn.init.zeros_(self.k_linear.bias)
        nn.init.zeros_(self.q_linear.bias)
        nn.init.xavier_uniform_(self.k_linear.weight)
        nn.init.xavier_uniform_(self.q_linear.weight)
        self.normalize_fact = float(hidden_dim / self.num_heads) ** -0.5

    def forward(self, q, k, mask=None):
        """q (B, Q, d), k (B, h*w, d) memory rows, mask (B, h*w) -> (B*Q, h*w, heads)."""
        if not fast_path(self):
            raise NotImplementedError('the segmentation head runs the inference path only (eval mode under '
                                      'torch.no_grad())')
        B, Q, d = q.shape
        qp = K.linear(q.reshape(B * Q, d), self.q_linear.weight, self.q_linear.bias)
        kp = K.linear(k.reshape(-1, d), self.k_linear.weight, self.k_linear.bias)
        return K.segm_attention(qp, kp.view(B, -1, self.hidden_dim), mask, Q, self.num_heads)

    def forward_autograd(self, q, k, mask=None):
        """forward on kinet_amd.autograd Functions (f32, differentiable): q (B, Q, d) ... -> (B*Q, h*w, heads)."""
        B, Q, d = q.shape
        qp = A.linear(q.reshape(B * Q, d), self.q_linear.weight, self.q_linear.bias)
        kp = A.linear(k.reshape(-1, d), self.k_linear.weight, self.k_linear.bias)
        return A.segm_attention(qp, kp.view(B, -1, self.hidden_dim), mask, Q, self.num_heads)


class MaskHeadSmallConv(nn.Module):
    """detr_segmentation.py:105-178, NHWC, lay1 split into its per-frame and per-query parts."""

    def __init__(self, dim, fpn_dims, context_dim):
        super().__init__()
        inter_dims = [dim, context_dim // 2, context_dim // 4, context_dim // 8, context_dim // 16, context_dim // 64]
        self.lay1 = nn.Conv2d(dim, dim, 3, padding=1)
        self.gn1 = nn.GroupNorm(8, dim)
        self.lay2 = nn.Conv2d(dim, inter_dims[1], 3, padding=1)
        self.gn2 = nn.GroupNorm(8, inter_dims[1])
        self.lay3 = nn.Conv2d(inter_dims[1], inter_dims[2], 3, padding=1)
        self.gn3 = nn.GroupNorm(8, inter_dims[2])
        self.lay4 = nn.Conv2d(inter_dims[2], inter_dims[3], 3, padding=1)
        self.gn4 = nn.GroupNorm(8, inter_dims[3])
        self.lay5 = nn.Conv2d(inter_dims[3], inter_dims[4], 3, padding=1)
        self.gn5 = nn.GroupNorm(8, inter_dims[4])
        self.out_lay = nn.Conv2d(inter_dims[4], 1, 3, padding=1)
        self.dim = dim
        self.adapter1 = nn.Conv2d(fpn_dims[0], inter_dims[1], 1)
        self.adapter2 = nn.Conv2d(fpn_dims[1], inter_dims[2], 1)
        self.adapter3 = nn.Conv2d(fpn_dims[2], inter_dims[3], 1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)

    # ---- per-frame operands
    def frame_part(self, src):
        """conv3x3(src; lay1.weight[:, :d]) + lay1.bias in f32: (B, h, w, d) -> (B, h, w, dim)."""
        d = src.shape[3]
        w = K.pack_segm_lay1_src(self.lay1.weight, d, torch.float32)
        # (src may be a strided view of the flattened transformer input: the convolution reads packed NHWC)
        return K.conv2d_nhwc(src.float().contiguous(), w, 1, 1, bias=K.f32(self.lay1.bias), ksplit=1)

    def adapters(self, fpns):
        """The three 1x1 adapters on the NHWC backbone features (layer3, layer2, layer1)."""
        out = []
        for ad, x in zip((self.adapter1, self.adapter2, self.adapter3), fpns):
            B, h, w, C = x.shape
            out.append(K.linear(x.view(B * h * w, C), K.param_matrix(ad.weight), ad.bias).view(B, h, w, -1))
        return out

    @staticmethod
    def _conv(x, conv):
        return K.conv2d_nhwc(x, K.pack_conv_weight(conv.weight, x.dtype), 1, 1, bias=K.f32(conv.bias), ksplit=1)

    @staticmethod
    def _gn(x, gn, fpn=None, row0=0, Q=None, row_frame=None):
        return K.segm_gn_relu(x, gn.weight, gn.bias, gn.num_groups, gn.eps, fpn=fpn, row0=row0, Q=Q,
                              row_frame=row_frame)

    def rows(self, att, frame, fpn_adapted, row0, Q, out, row_frame=None):
        """The head for rows [row0, row0 + n) of the B*Q rows: att (n, h, w, heads) -> out (n, H, W) f32.
        With row_frame (n, device int32) the rows are a ragged list and row r reads frame row_frame[r]."""
        d = self.dim - att.shape[3]
        x = K.segm_lay1(att, K.segm_lay1_weights(self.lay1.weight, d), frame, row0, Q, row_frame=row_frame)
        x = self._gn(x, self.gn1)
        x = self._conv(x, self.lay2)
        # the first "interpolate" (:156) maps stride 16 onto stride 16: the identity of the same entry point
        x = self._gn(x, self.gn2, fpn_adapted[0], row0, Q, row_frame)
        x = self._conv(x, self.lay3)
        x = self._gn(x, self.gn3, fpn_adapted[1], row0, Q, row_frame)
        x = self._conv(x, self.lay4)
        x = self._gn(x, self.gn4, fpn_adapted[2], row0, Q, row_frame)
        x = self._conv(x, self.lay5)
        x = self._gn(x, self.gn5)
        return K.segm_out_conv(x, K.segm_out_weights(self.out_lay.weight), K.f32(self.out_lay.bias), out=out)

    def forward_autograd(self, src, att, fpns, Q):
        """forward on kinet_amd.autograd Functions (f32, differentiable w.r.t. every input and
        parameter), all rows in one pass: the training head's recompute on the matched rows."""
        d = self.dim - att.shape[3]
        n, h, w, _ = att.shape

        def gn(x, mod):
            r, hh, ww, C = x.shape
            return A.group_norm_nhwc(x.reshape(r, hh * ww, C), mod).view(r, hh, ww, C)

        def conv(x, mod):
            return A.conv_nhwc(x, mod.weight, mod.bias, 1, 1)
        adapted = []
        for ad, f in zip((self.adapter1, self.adapter2, self.adapter3), fpns):
            B, fh, fw, C = f.shape
            adapted.append(A.linear(f.reshape(B * fh * fw, C), ad.weight.view(ad.out_channels, C), ad.bias)
                           .view(B, fh, fw, -1))
        frame = A.conv_nhwc(src, self.lay1.weight[:, :d], self.lay1.bias, 1, 1)        # (B, h, w, dim)
        x = A.conv_nhwc(att, self.lay1.weight[:, d:], None, 1, 1)
        x = (x.view(-1, Q, h, w, self.dim) + frame.unsqueeze(1)).view(n, h, w, self.dim)
        x = A.segm_relu_up_add(gn(x, self.gn1))
        x = conv(x, self.lay2)
        x = A.segm_relu_up_add(gn(x, self.gn2), adapted[0], 0, Q)
        x = conv(x, self.lay3)
        x = A.segm_relu_up_add(gn(x, self.gn3), adapted[1], 0, Q)
        x = conv(x, self.lay4)
        x = A.segm_relu_up_add(gn(x, self.gn4), adapted[2], 0, Q)
        x = conv(x, self.lay5)
        x = A.segm_relu_up_add(gn(x, self.gn5))
        return A.segm_out_conv(x, self.out_lay.weight, self.out_lay.bias)

    def forward(self, src, att, fpns, Q, chunk=None):
        """src (B, h, w, d) NHWC, att (B*Q, h, w, heads), fpns NHWC backbone features [layer3, layer2,
        layer1] -> (B*Q, H/4, W/4) f32 logits."""
        if not fast_path(self):
            raise NotImplementedError('the segmentation head runs the inference path only (eval mode under '
                                      'torch.no_grad())')
        return self.run(att, self.frame_part(src), self.adapters(fpns), Q, chunk)

    def run(self, att, frame, adapted, Q, chunk=None, row_frame=None):
        """The head over all rows of att in chunks, on per-frame operands that are already computed.
        row_frame (rows, device int32): the rows' frames when they are a ragged list (Q is then not used);
        a chunk takes its slice of the list."""
        R = att.shape[0]
        H, W = adapted[2].shape[1:3]
        out = torch.empty((R, H, W), dtype=torch.float32, device=att.device)
        if chunk is None:
            # the largest pair of live activations of a row: lay5's input and output at stride 4, and
            # lay4's pair one level down
            c4, c5 = self.lay4.out_channels, self.lay5.out_channels
            per_row = H * W * (2 * c4 + c5) * att.element_size()
            chunk = max(1, MASK_WORKSPACE_BYTES // max(per_row, 1))
        chunk = max(1, min(int(chunk), 65535))
        for r0 in range(0, R, chunk):
            r1 = min(R, r0 + chunk)
            self.rows(att[r0:r1], frame, adapted, r0, Q, out[r0:r1],
                      None if row_frame is None else row_frame[r0:r1])
        return out


class _MaskHeadTrain(torch.autograd.Function):
    """pred_masks of the training forward (module docstring): the inference head over all rows
    forward, the differentiable head recomputed on the rows with a non-zero incoming gradient
    backward.  Inputs after (model, mask): hs (B, Q, d), k_rows (B, h*w, d), src (B, h, w, d), the
    three NHWC FPN features, then the head's parameters (so that autograd routes their gradients)."""

    N_IN = 6

    @staticmethod
    def forward(ctx, model, mask, *tensors):
        inputs = [t.detach() for t in tensors[:_MaskHeadTrain.N_IN]]
        hs, k_rows, src = inputs[:3]
        fpns = [f.contiguous() for f in inputs[3:]]
        B, Q, d = hs.shape
        h, w = src.shape[1:3]
        att_mod, head = model.bbox_attention, model.mask_head
        qp = K.linear(hs.reshape(B * Q, d), att_mod.q_linear.weight, att_mod.q_linear.bias)
        kp = K.linear(k_rows.reshape(-1, d), att_mod.k_linear.weight, att_mod.k_linear.bias)
        att = K.segm_attention(qp, kp.view(B, -1, att_mod.hidden_dim), mask, Q, att_mod.num_heads)
        seg = head.run(att.view(B * Q, h, w, -1), head.frame_part(src), head.adapters(fpns), Q, model.mask_query_chunk)
        ctx.save_for_backward(*inputs)
        ctx.model, ctx.mask = model, mask
        ctx.params = tensors[_MaskHeadTrain.N_IN:]
        return seg.view(B, Q, seg.shape[-2], seg.shape[-1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dseg):
        model, mask, params = ctx.model, ctx.mask, ctx.params
        inputs = ctx.saved_tensors
        n_in = _MaskHeadTrain.N_IN
        B, Q = dseg.shape[:2]
        dseg = dseg.contiguous().float()
        if model.mask_train_all_rows:
            rows = [list(range(Q))] * B
        else:
            # the one host sync of the head's backward: which rows carry a gradient at all
            live = (dseg.flatten(2) != 0).any(2).tolist()
            rows = [[q for q in range(Q) if live[b][q]] for b in range(B)]
        model.last_mask_rows = rows
        need_in = ctx.needs_input_grad[2:2 + n_in]
        need_p = ctx.needs_input_grad[2 + n_in:]
        g_in = [None] * n_in
        g_p = [None] * len(params)
        for b, idx in enumerate(rows):
            if not idx:
                continue
            idx_t = torch.tensor(idx, dtype=torch.int64, device=dseg.device)
            leaves = [inputs[0][b].index_select(0, idx_t).unsqueeze(0)] + [t[b:b + 1] for t in inputs[1:]]
            leaves = [t.detach().requires_grad_(bool(nd)) for t, nd in zip(leaves, need_in)]
            with torch.enable_grad():
                out = model._mask_rows_autograd(leaves[0], leaves[1], mask[b:b + 1], leaves[2], leaves[3:])
            wanted = [(g_in, i, t) for i, (t, nd) in enumerate(zip(leaves, need_in)) if nd]
            wanted += [(g_p, i, p) for i, (p, nd) in enumerate(zip(params, need_p)) if nd]
            grads = torch.autograd.grad(out, [t for _, _, t in wanted], dseg[b].index_select(0, idx_t),
                                        allow_unused=True)
            for (store, i, _), g in zip(wanted, grads):
                if g is None:
                    continue
                if store is g_in:
                    if g_in[i] is None:
                        g_in[i] = torch.zeros_like(inputs[i])
                    if i == 0:
                        g_in[0][b].index_copy_(0, idx_t, g[0])
                    else:
                        g_in[i][b:b + 1] = g
                else:       # the frames in ascending order
                    g_p[i] = g if g_p[i] is None else g_p[i] + g
        return (None, None) + tuple(g_in) + tuple(g_p)


class DETRSegmBase(nn.Module):
    def __init__(self, freeze_detr=False):
        if freeze_detr:
            for param in self.parameters():
                param.requires_grad_(False)
        if getattr(self, 'two_stage', False):
            raise NotImplementedError('masks with two_stage is not built')
        if self.num_feature_levels != 4 or len(self.backbone.num_channels) != 4:
            # input_proj[-3] must be the projection of features[-2] (detr_segmentation.py:45-48)
            raise NotImplementedError('the segmentation head needs the 4-level detector over all four backbone layers '
                                      '(masks: true sets return_interm_layers)')
        nheads = self.transformer.nhead
        self.bbox_attention = MHAttentionMap(self.hidden_dim, self.hidden_dim, nheads, dropout=0.0)
        self.mask_head = MaskHeadSmallConv(self.hidden_dim + nheads, self.fpn_channels, self.hidden_dim)
        self.mask_query_chunk = None    # rows of (frame, query) per pass of the head; None = by workspace bound
        self.keep_attention = False     # True: keep the last attention map as self.last_attention
        self.last_attention = None
        self.defer_masks = False        # True: forward returns no 'pred_masks'; mask_logits(rows) runs the head
        self._mask_ctx = None           # the last deferred forward's operands, valid until the next forward
        self.mask_training = False      # True (train.build_mask_training): off the fast path, run the training forward
        self.mask_train_all_rows = False   # diagnostic: back-propagate the head over all B*Q rows, not the live ones
        self.last_mask_rows = None      # per frame, the query rows the last head backward ran on

    @property
    def fpn_channels(self):
        """detr.py:61-64."""
        return self.backbone.num_channels[:3][::-1]

    def _mask_rows_autograd(self, hs_rows, k_rows, mask, src, fpns):
        """The differentiable head for the rows hs_rows (1, n, d) of ONE frame (k_rows, mask, src and fpns
        are that frame's, batch 1) -> (n, H/4, W/4) logits."""
        n = hs_rows.shape[1]
        h, w = src.shape[1:3]
        att = self.bbox_attention.forward_autograd(hs_rows, k_rows, mask)
        return self.mask_head.forward_autograd(src, att.view(n, h, w, -1), fpns, n)

    def _forward_train(self, samples, targets, prev_features):
        """The training forward (module docstring): detector on _forward_reference, pred_masks from
        _MaskHeadTrain.  One host sync per step in the head's backward (the rows that carry a gradient)."""
        self._segm_want = True
        try:
            out, targets, features, memory, hs = super().forward(samples, targets, prev_features)
            ctx = self._segm_ctx
        finally:
            self._segm_want = False
            self._segm_ctx = None
        # detr_segmentation.py:44-53; src = input_proj[-3](features[-2]) is the tensor the transformer
        # read (the reference computes it a second time: the same values, the same gradient sum)
        src = ctx['src_nchw'].permute(0, 2, 3, 1)
        mask = ctx['mask'].flatten(1)
        fpns = [features[i].tensors.permute(0, 2, 3, 1) for i in (-2, -3, -4)]
        memory = memory[-3]
        if tuple(memory.shape[-2:]) != tuple(src.shape[1:3]) or mask.shape[1] != src.shape[1] * src.shape[2]:
            raise RuntimeError('segmentation head: memory level and layer-3 feature differ in size')
        k_rows = memory.flatten(2).permute(0, 2, 1)
        params = list(self.bbox_attention.parameters()) + list(self.mask_head.parameters())
        self._mask_ctx = None
        out['pred_masks'] = _MaskHeadTrain.apply(self, mask, hs[-1].float(), k_rows.float(), src.float(),
                                                 *[f.float() for f in fpns], *params)
        return out, targets, features, memory, hs

    def forward(self, samples, targets: list = None, prev_features=None):
        if not fast_path(self):
            if self.mask_training:
                return self._forward_train(samples, targets, prev_features)
            raise NotImplementedError('DeformableDETRSegm runs the inference path only (eval mode under '
                                      'torch.no_grad()) unless mask_training is set: '
                                      'kinet_amd.train.build_mask_training builds the model and criterion that train')
        self._segm_want = True
        try:
            out, targets, features, memory, hs = super().forward(samples, targets, prev_features)
            ctx = self._segm_ctx
        finally:
            self._segm_want = False
            self._segm_ctx = None
        # detr_segmentation.py:44-53.  src = input_proj[-3](features[-2]): the current frame's level 1
        # of the flattened transformer input (the transformer writes new tensors, the buffer is intact)
        B, d = hs.shape[1], self.hidden_dim
        h, w = ctx['shapes'][1]
        off = ctx['offsets'][1]
        src = ctx['src'][:, off:off + h * w].reshape(B, h, w, d)
        mask = ctx['masks'][-2]
        feats = ctx['feats']
        fpns = [feats[-2], feats[-3], feats[-4]]
        memory = memory[-3]
        if tuple(memory.shape[-2:]) != (h, w) or tuple(mask.shape[-2:]) != (h, w):
            raise RuntimeError('segmentation head: memory level and layer-3 feature differ in size')
        Q = hs.shape[2]
        k_rows = memory.flatten(2).permute(0, 2, 1)                       # (B, h*w, d) rows of the level
        self._mask_ctx = None
        if self.defer_masks:
            self._mask_ctx = {'hs': hs[-1], 'k_rows': k_rows, 'mask': mask.flatten(1), 'src': src, 'fpns': fpns,
                              'hw': (h, w)}
            return out, targets, features, memory, hs
        att = self.bbox_attention(hs[-1], k_rows, mask.flatten(1))        # (B*Q, h*w, heads)
        att = att.view(B * Q, h, w, -1)
        if self.keep_attention:
            self.last_attention = att.view(B, Q, h, w, -1).permute(0, 1, 4, 2, 3)   # the reference's (B, Q, heads, h, w)
        seg = self.mask_head(src, att, fpns, Q, self.mask_query_chunk)
        out['pred_masks'] = seg.view(B, Q, seg.shape[-2], seg.shape[-1])
        return out, targets, features, memory, hs

    @torch.no_grad()
    def mask_logits(self, rows, frame=0):
        """pred_masks[frame, rows] of the last forward run with defer_masks: rows is a device int64
        tensor of query rows (any order, repeats allowed) -> (len(rows), H/4, W/4) f32, bit-identical
        to the rows of the full head.  The per-frame operands (k_linear of the level, lay1's frame
        part, the adapters) and q_linear over ALL rows are computed at the first call after a forward,
        by the calls the full head makes, so no GEMM sees another shape than there; the attention map
        and the head then run on the chosen rows as one frame of len(rows) queries."""
        ctx = self._mask_ctx
        if ctx is None:
            raise RuntimeError('mask_logits needs a forward with defer_masks set (and none since without it)')
        hs = ctx['hs']
        B, Q, d = hs.shape
        if not 0 <= int(frame) < B:
            raise IndexError(f'mask_logits: frame {frame} outside the {B} frames of the last forward')
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise RuntimeError('mask_logits: rows must be a 1-d int64 tensor')
        n = rows.numel()
        if n == 0:      # (no launch: the stride-4 backbone feature has the logits' size)
            return torch.empty((0,) + tuple(ctx['fpns'][2].shape[1:3]), dtype=torch.float32, device=hs.device)
        if 'qp' not in ctx:
            att_mod = self.bbox_attention
            ctx['qp'] = K.linear(hs.reshape(B * Q, d), att_mod.q_linear.weight, att_mod.q_linear.bias)
            ctx['kp'] = K.linear(ctx['k_rows'].reshape(-1, d), att_mod.k_linear.weight,
                                 att_mod.k_linear.bias).view(B, -1, att_mod.hidden_dim)
            ctx['frame'] = self.mask_head.frame_part(ctx['src'])
            ctx['adapted'] = self.mask_head.adapters(ctx['fpns'])
        b = int(frame)
        h, w = ctx['hw']
        qp = ctx['qp'].view(B, Q, -1)[b].index_select(0, rows.to(hs.device))
        att = K.segm_attention(qp, ctx['kp'][b:b + 1], ctx['mask'][b:b + 1], n, self.bbox_attention.num_heads)
        att = att.view(n, h, w, -1)
        return self.mask_head.run(att, ctx['frame'][b:b + 1], [a[b:b + 1] for a in ctx['adapted']], n,
                                  self.mask_query_chunk)

    def _mask_operands(self, ctx):
        """The per-frame operands of the deferred head, computed once per forward (mask_logits' statements)."""
        if 'qp' not in ctx:
            hs = ctx['hs']
            B, Q, d = hs.shape
            att_mod = self.bbox_attention
            ctx['qp'] = K.linear(hs.reshape(B * Q, d), att_mod.q_linear.weight, att_mod.q_linear.bias)
            ctx['kp'] = K.linear(ctx['k_rows'].reshape(-1, d), att_mod.k_linear.weight,
                                 att_mod.k_linear.bias).view(B, -1, att_mod.hidden_dim)
            ctx['frame'] = self.mask_head.frame_part(ctx['src'])
            ctx['adapted'] = self.mask_head.adapters(ctx['fpns'])
        return ctx

    @torch.no_grad()
    def mask_logits_rows(self, rows, frames):
        """pred_masks[frames[i], rows[i]] of the last forward run with defer_masks, for rows of ANY frames in
        one pass of the head: rows a device int64 tensor of query rows, frames a device int32 tensor of the
        same length (each in [0, B); a row whose frame is outside is left unwritten by the kernels) ->
        (len(rows), H/4, W/4) f32.  Bit-identical to mask_logits(rows[frames == b], b) for every b: the
        per-frame operands are mask_logits' (shared with it), q_linear's rows are gathered at
        frames * Q + rows, and the attention map and the head run once over all rows through the ragged
        entry points (kinet_segm_*_rows), whose kernels are the frame-major ones."""
        ctx = self._mask_ctx
        if ctx is None:
            raise RuntimeError('mask_logits_rows needs a forward with defer_masks set (and none since without it)')
        hs = ctx['hs']
        B, Q, d = hs.shape
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise RuntimeError('mask_logits_rows: rows must be a 1-d int64 tensor')
        if frames.dtype != torch.int32 or frames.dim() != 1 or frames.numel() != rows.numel():
            raise RuntimeError('mask_logits_rows: frames must be a 1-d int32 tensor, one frame per row')
        n = rows.numel()
        if n == 0:      # (no launch)
            return torch.empty((0,) + tuple(ctx['fpns'][2].shape[1:3]), dtype=torch.float32, device=hs.device)
        self._mask_operands(ctx)
        h, w = ctx['hw']
        frames = frames.to(hs.device).contiguous()
        qp = ctx['qp'].index_select(0, frames.to(torch.int64) * Q + rows.to(hs.device))
        att = K.segm_attention_rows(qp, ctx['kp'], ctx['mask'], frames, self.bbox_attention.num_heads)
        att = att.view(n, h, w, -1)
        return self.mask_head.run(att, ctx['frame'], ctx['adapted'], 1, self.mask_query_chunk, row_frame=frames)


class DeformableDETRSegm(DETRSegmBase, DeformableDETR):
    def __init__(self, mask_kwargs, detr_kwargs):
        DeformableDETR.__init__(self, **detr_kwargs)
        DETRSegmBase.__init__(self, **mask_kwargs)


class DeformableDETRSegmTracking(DETRSegmBase, DETRTrackingBase, DeformableDETR):
    def __init__(self, mask_kwargs, tracking_kwargs, detr_kwargs):
        DeformableDETR.__init__(self, **detr_kwargs)
        DETRTrackingBase.__init__(self, **tracking_kwargs)
        DETRSegmBase.__init__(self, **mask_kwargs)


class PostProcessSegm(nn.Module):
    """detr_segmentation.py:219-253 on kinet_segm_postprocess: per frame, bilinear resize of the
    logits to max_target_sizes.max(0), sigmoid, crop to the frame's size, nearest resize to its
    original size -- in one kernel, the full-resolution intermediate is never materialised.
    Returns CPU tensors like the reference; on_device=True leaves them on the GPU (no sync when the
    size tensors live on the host)."""

    def __init__(self, threshold=0.5):
        super().__init__()
        self.threshold = threshold

    @torch.no_grad()
    def forward(self, results, outputs, orig_target_sizes, max_target_sizes, return_probs=False, results_mask=None,
                on_device=False):
        assert len(orig_target_sizes) == len(max_target_sizes)
        max_h, max_w = max_target_sizes.max(0)[0].tolist()
        masks_all = outputs['pred_masks'].squeeze(2)
        sizes = torch.as_tensor(max_target_sizes).tolist()
        origs = torch.as_tensor(orig_target_sizes).tolist()
        for i, (logits, t, tt) in enumerate(zip(masks_all, sizes, origs)):
            masks = K.segm_postprocess(logits, (max_h, max_w), (t[0], t[1]), (tt[0], tt[1]), self.threshold,
                                       return_probs)
            if results_mask is not None:
                masks = masks[results_mask[i]]
            results[i]['masks'] = masks if on_device else masks.cpu()
        return results
