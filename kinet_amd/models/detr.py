"""Vanilla DETR detector (src/trackformer/models/detr.py:17-149, the reference's default
configuration: cfgs/train.yaml has `deformable: false`) on the kinet_amd kernels.

Same module / parameter names as the reference (`transformer.*`, `class_embed`, `bbox_embed`,
`query_embed`, `input_proj` -- a bare Conv2d here, not DeformableDETR's ModuleList --,
`backbone.0.body.*`), same forward signature `model(samples, targets=None, prev_features=None)
-> (out, targets, features, memory, hs)` and output dict keys.

Inference (autograd off, eval mode) is the kernel path: ResNet body NHWC, the 1x1 input
projection as a GEMM, the sine embedding kernel, q|k projections with the position embedding as
the GEMM's second operand, the dense attention core (`kernels.mha_core`: all H*W keys, so the
key-streaming MFMA kernel in the 16-bit modes once H*W exceeds the resident kernels' caps), the
fused out-projection / FFN launches, the heads as GEMMs.  What depends on the frame geometry only
(the flattened padding mask as bytes, the position embedding) is cached per geometry.

Training (autograd on; or train mode with active dropout under torch.no_grad() inside
reference_path(), as DETRTrackingBase runs the previous frame -- outside it that combination still
raises: it is a forgotten eval()) is the same graph in f32 on the kinet_amd.autograd
Functions: the differentiable backbone (stage-4 feature only, as the reference), the input projection
as a Linear, the same sine rows, `transformer.run(..., fast=False)` -- whose dense attentions run the
key-streaming f32 MFMA pair `autograd.mha_core_stream` (csrc/attn_train.hip) --, the heads as Linear
Functions.  Track queries in `targets` stay differentiable.  Same output dict, tuple and aux outputs.
"""
import torch
from torch import nn

from kinet_amd import autograd as A
from kinet_amd import kernels as K
from kinet_amd.models.backbone import interp_mask, nhwc_as_nchw
from kinet_amd.models.deformable_detr import MLP
from kinet_amd.models.deformable_transformer import fast_path, in_reference_path, mlp_fast
from kinet_amd.models.misc import NestedTensor, nested_tensor_from_tensor_list


class DETR(nn.Module):
    def __init__(self, backbone, transformer, num_classes, num_queries, aux_loss=False, overflow_boxes=False,
                 multi_frame_encoding=False, multi_frame_attention=False, merge_frame_features=False):
        super().__init__()
        if multi_frame_encoding and multi_frame_attention:
            # detr.py:120-123 calls .flatten on a list: the reference raises there as shipped
            raise NotImplementedError('vanilla DETR with multi_frame_encoding + multi_frame_attention '
                                      '(broken in the reference, detr.py:120-123)')
        # detr.py:35-53, same registration order
        self.num_queries = num_queries
        self.transformer = transformer
        self.overflow_boxes = overflow_boxes
        self.class_embed = nn.Linear(self.hidden_dim, num_classes + 1)
        self.bbox_embed = MLP(self.hidden_dim, self.hidden_dim, 4, 3)
        self.query_embed = nn.Embedding(num_queries, self.hidden_dim)
        self.input_proj = nn.Conv2d(backbone.num_channels[-1], self.hidden_dim, kernel_size=1)
        self.backbone = backbone
        self.aux_loss = aux_loss
        self.multi_frame_encoding = multi_frame_encoding
        self.multi_frame_attention = multi_frame_attention
        self.merge_frame_features = merge_frame_features
        self.compute_dtype = torch.float32
        self._geo_cache = {}

    @property
    def hidden_dim(self):
        return self.transformer.d_model

    def set_compute_dtype(self, dtype):
        """torch.bfloat16 / torch.float16 (perf) or torch.float32 (parity) for the inference path."""
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f'unsupported compute dtype {dtype}')
        self.compute_dtype = dtype
        self._geo_cache.clear()
        return self

    def _geometry(self, samples, hw, dtype=None):
        """(padding mask at the feature resolution, the same flattened as bytes for the attention
        kernels, position embedding rows (B, H*W, d) in `dtype`, default the compute dtype); cached
        per image sizes when they determine the mask (NestedTensor.sizes)."""
        dtype = self.compute_dtype if dtype is None else dtype
        key = None if samples.sizes is None else (samples.sizes, tuple(samples.mask.shape), hw, dtype,
                                                  str(samples.mask.device))
        geo = self._geo_cache.get(key) if key is not None else None
        if geo is None:
            mask = interp_mask(samples.mask, hw)
            pos = self.backbone[1].rows(mask, out_dtype=dtype)
            geo = (mask, mask.flatten(1).to(torch.uint8).contiguous(), pos.view(mask.shape[0], hw[0] * hw[1], -1))
            if key is not None:
                if len(self._geo_cache) > 16:
                    self._geo_cache.clear()
                self._geo_cache[key] = geo
        return geo

    def forward(self, samples, targets: list = None, prev_features=None):
        if targets is not None and len(targets) and 'track_queries_placeholder_mask' in targets[0]:
            raise NotImplementedError('vanilla DETR does not take ragged track queries '
                                      '(track_queries_placeholder_mask): the Deformable detector does')
        if not isinstance(samples, NestedTensor):
            samples = nested_tensor_from_tensor_list(samples)
        if not fast_path(self):
            if not (torch.is_grad_enabled() or in_reference_path()):
                # a bare train-mode call with active dropout and no autograd: most likely a missing eval()
                raise NotImplementedError('vanilla DETR in train mode with active dropout under torch.no_grad(): call '
                                          'eval() for the inference kernels; the no-grad previous-frame pass of '
                                          'training enters through reference_path()')
            return self._forward_train(samples, targets)
        dt = self.compute_dtype
        device = samples.tensors.device
        feats = self.backbone[0].forward_nhwc(samples.tensors, dt)      # [layer4] NHWC
        x = feats[-1]
        B, h, w, C = x.shape
        d = self.hidden_dim
        mask, mask_bytes, pos = self._geometry(samples, (h, w))
        features = [NestedTensor(nhwc_as_nchw(f), mask, samples.sizes) for f in feats]
        proj = self.input_proj
        src = K.linear(x.view(B * h * w, C), K.param_matrix(proj.weight), proj.bias).view(B, h * w, d)

        query_embed = K.weight_as(self.query_embed.weight, dt)[None].expand(B, -1, -1)
        if targets is not None and 'track_query_hs_embeds' in targets[0]:
            # detr.py:99-117: K track queries in front, zero query positions, their embeddings as tgt
            track = torch.stack([t['track_query_hs_embeds'] for t in targets]).to(dt)
            n_track = track.shape[1]
            query_embed = torch.cat([torch.zeros((B, n_track, d), dtype=dt, device=device), query_embed], 1)
            tgt = torch.cat([track, torch.zeros((B, self.num_queries, d), dtype=dt, device=device)], 1)
            for i, target in enumerate(targets):
                target['track_query_hs_embeds'] = tgt[i].float()
        else:
            query_embed = query_embed.contiguous()
            tgt = torch.zeros_like(query_embed)

        hs, hs_without_norm, memory = self.transformer.run(src, mask_bytes, query_embed, pos, tgt)

        outputs_class = K.linear(hs, self.class_embed.weight, self.class_embed.bias, out_dtype=torch.float32)
        outputs_coord = mlp_fast(self.bbox_embed, hs).sigmoid()
        out = {'pred_logits': outputs_class[-1], 'pred_boxes': outputs_coord[-1],
               'hs_embed': hs_without_norm[-1].float()}
        if self.aux_loss:
            out['aux_outputs'] = self._set_aux_loss(outputs_class, outputs_coord)
        return out, targets, features, memory.permute(0, 2, 1).view(B, d, h, w), hs

    def _forward_train(self, samples, targets):
        """detr.py:66-141 in f32 on the kinet_amd.autograd Functions (module docstring)."""
        if samples.tensors.device.type != 'cuda':
            raise NotImplementedError('vanilla DETR has no CPU path: inference and training both run the HIP kernels, '
                                      'move the model and the samples to the GPU')
        body = self.backbone[0]
        xs = body.body.forward_autograd(samples.tensors.float())
        feats = [xs[str(i)] for i in body.return_idx]                   # NCHW views of NHWC buffers
        x = feats[-1].permute(0, 2, 3, 1)
        B, h, w, C = x.shape
        d = self.hidden_dim
        mask, mask_bytes, pos = self._geometry(samples, (h, w), torch.float32)
        features = [NestedTensor(f, mask if f is feats[-1] else interp_mask(samples.mask, f.shape[-2:]), samples.sizes)
                    for f in feats]
        proj = self.input_proj
        src = A.linear(x.reshape(B * h * w, C), proj.weight.view(d, C), proj.bias).view(B, h * w, d)

        query_embed = self.query_embed.weight[None].expand(B, -1, -1)
        if targets is not None and 'track_query_hs_embeds' in targets[0]:
            # detr.py:99-117, differentiable w.r.t. the track embeddings
            track = torch.stack([t['track_query_hs_embeds'] for t in targets]).float()
            n_track = track.shape[1]
            query_embed = torch.cat([query_embed.new_zeros((B, n_track, d)), query_embed], 1)
            tgt = torch.cat([track, track.new_zeros((B, self.num_queries, d))], 1)
            for i, target in enumerate(targets):
                target['track_query_hs_embeds'] = tgt[i]
        else:
            tgt = torch.zeros((B, self.num_queries, d), dtype=torch.float32, device=x.device)

        hs, hs_without_norm, memory = self.transformer.run(src, mask_bytes, query_embed, pos, tgt, fast=False)

        outputs_class = A.linear_module(hs, self.class_embed)
        outputs_coord = self.bbox_embed(hs).sigmoid()
        out = {'pred_logits': outputs_class[-1], 'pred_boxes': outputs_coord[-1], 'hs_embed': hs_without_norm[-1]}
        if self.aux_loss:
            out['aux_outputs'] = self._set_aux_loss(outputs_class, outputs_coord)
        return out, targets, features, memory.permute(0, 2, 1).view(B, d, h, w), hs

    @torch.jit.unused
    def _set_aux_loss(self, outputs_class, outputs_coord):
        return [{'pred_logits': a, 'pred_boxes': b} for a, b in zip(outputs_class[:-1], outputs_coord[:-1])]
