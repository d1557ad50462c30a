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
(the flattened padding mask as bytes, the position embedding) is cached per geometry.  Training
of vanilla DETR is not built: a forward with autograd on or active dropout raises.
"""
import torch
from torch import nn

from kinet_amd import kernels as K
from kinet_amd.models.backbone import interp_mask, nhwc_as_nchw
from kinet_amd.models.deformable_detr import MLP
from kinet_amd.models.deformable_transformer import fast_path, mlp_fast
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

    def _geometry(self, samples, hw):
        """(padding mask at the feature resolution, the same flattened as bytes for the attention
        kernels, position embedding rows (B, H*W, d) in the compute dtype); cached per image
        sizes when they determine the mask (NestedTensor.sizes)."""
        key = None if samples.sizes is None else (samples.sizes, tuple(samples.mask.shape), hw, self.compute_dtype,
                                                  str(samples.mask.device))
        geo = self._geo_cache.get(key) if key is not None else None
        if geo is None:
            mask = interp_mask(samples.mask, hw)
            pos = self.backbone[1].rows(mask, out_dtype=self.compute_dtype)
            geo = (mask, mask.flatten(1).to(torch.uint8).contiguous(), pos.view(mask.shape[0], hw[0] * hw[1], -1))
            if key is not None:
                if len(self._geo_cache) > 16:
                    self._geo_cache.clear()
                self._geo_cache[key] = geo
        return geo

    def forward(self, samples, targets: list = None, prev_features=None):
        if not isinstance(samples, NestedTensor):
            samples = nested_tensor_from_tensor_list(samples)
        if not fast_path(self):
            raise NotImplementedError('vanilla DETR runs the inference kernels only: call it in eval mode under '
                                      'torch.no_grad() (training config 1 is not built)')
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

    @torch.jit.unused
    def _set_aux_loss(self, outputs_class, outputs_coord):
        return [{'pred_logits': a, 'pred_boxes': b} for a, b in zip(outputs_class[:-1], outputs_coord[:-1])]
