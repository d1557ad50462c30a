"""Vanilla DETR transformer (src/trackformer/models/transformer.py:19-84, `build_transformer`
:503-537) on kinet_amd kernels: a post-norm encoder over the flattened stride-32 feature map and
a post-norm decoder over the object (+ track) queries.

The layers are the post-norm classes of kinet_amd/models/kinet.py (the reference shares them
between its image and kinematic transformers too); module names and parameter shapes equal the
reference's (`encoder.layers.N.*`, `decoder.layers.N.*`, `decoder.norm`).  Both attentions are
dense over all H*W keys (1050 at 800x1333), which is what the key-streaming MFMA kernel of
csrc/attn.hip is for.  Batch-first (B, L, d) throughout.

`run` is the interface: the inference kernels with fast=True, the kinet_amd.autograd Functions (f32,
differentiable, the reference's dropouts) with fast=False.  The layers carry `dense_attn`, so in
training both attentions run the key-streaming f32 MFMA pair `autograd.mha_core_stream`
(csrc/attn_train.hip) where its planner takes the shape (csrc/attn_train_plan.h); KineT's layers, of
the same classes, keep `autograd.mha_core`.  Pre-norm, non-ReLU activations and `track_attention`
(false in every shipped config) raise at construction.
"""
from torch import nn

from kinet_amd.models.kinet import (TransformerDecoder, TransformerDecoderLayer, TransformerEncoder,
                                    TransformerEncoderLayer)


class Transformer(nn.Module):
    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=2048,
                 dropout=0.1, activation='relu', normalize_before=False, return_intermediate_dec=False,
                 track_attention=False):
        super().__init__()
        if track_attention:
            raise NotImplementedError('track_attention (false in every config)')
        if normalize_before or activation != 'relu':
            raise NotImplementedError('pre-norm / non-ReLU transformer layers (false in every config)')
        enc = TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation, normalize_before)
        dec = TransformerDecoderLayer(d_model, nhead, dim_feedforward, dropout, activation, normalize_before)
        enc.fused_ffn = dec.fused_ffn = True   # instance attributes: the clones carry them
        enc.dense_attn = dec.dense_attn = True
        self.encoder = TransformerEncoder(enc, num_encoder_layers)
        self.decoder = TransformerDecoder(dec, num_decoder_layers, d_model, return_intermediate_dec)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.d_model = d_model
        self.nhead = nhead

    def run(self, src, mask, query_embed, pos, tgt, fast=True):
        """src / pos (B, HW, d), mask (B, HW) uint8 or bool (True = padding), query_embed / tgt
        (B, Q, d) -> hs (layers, B, Q, d) after the decoder norm, the same before it, memory
        (B, HW, d).  fast=False: the differentiable f32 graph (module docstring)."""
        memory = self.encoder.run(src, pos, mask, fast)
        hs, hs_without_norm = self.decoder.run(tgt, memory, pos, query_embed, mask, fast)
        return hs, hs_without_norm, memory

    def forward(self, *args, **kwargs):
        raise NotImplementedError('Transformer is driven by DETR.forward through run()')


def build_transformer(args):
    """transformer.py:526-537 (the image branch; the kinematic ones are kinet.build_kinet)."""
    return Transformer(d_model=args.hidden_dim, nhead=args.nheads, num_encoder_layers=args.enc_layers,
                       num_decoder_layers=args.dec_layers, dim_feedforward=args.dim_feedforward,
                       dropout=args.dropout, activation=args.activation, normalize_before=args.pre_norm,
                       return_intermediate_dec=True, track_attention=args.track_attention)
