"""The constants, frames, targets and gates that the vanilla-DETR training fixture
(tests/golden/make_golden_detr_train.py -> detr_vanilla_train.npz) and its test
(tests/test_detr_train_gpu.py) share.

Setup: cfgs/train.yaml as shipped (vanilla, focal_loss false, aux_loss true, 100 queries, d = 256) with
dropout 0 and 2 encoder + 2 decoder layers, train mode; two frames of different sizes in one NestedTensor,
3x384x480 and 3x320x416: a 12x15 stride-32 map = 180 keys (more than one 64-key tile of the training
attention), 50 of the second frame's keys padded; 3 and 2 target boxes.  Frames, targets, the track-query
embeddings and the loss weights of the criterion-free case come from seeds: only results are stored.

Gates (the form of tests/test_two_stage_train_gpu.py, through tests/segm_train_refs.py): a gradient within
2e-3 max|ref| + 1e-5 (5e-3 for a backbone weight), a loss within 1e-3 relative + 1e-4, the outputs of the
track-query case within 1e-3 max|ref| + 1e-4.  The generator
asserts that 10 x the reference's own f32-vs-f64 difference (stored as err64:<name>) lies under each: the
constants are a margin over the reference's f32 rounding, not over what the code under test reaches."""
import torch

from segm_train_refs import GRAD_ATOL, GRAD_GATE, GRAD_GATE_BACKBONE, grad_gate, lattice  # noqa: F401  (shared gates)

LOSS_RTOL, LOSS_ATOL = 1e-3, 1e-4

FRAMES = ((3101, 384, 480), (3102, 320, 416))            # (generator seed, H, W)
MAP_HW, KEYS, PADDED_KEYS = (12, 15), 180, 50
OVER = dict(dropout=0.0, enc_layers=2, dec_layers=2)
TARGETS = ((6101, 3), (6102, 2))                         # (generator seed, boxes) per frame
GRADS = ('backbone.0.body.layer2.0.conv1.weight', 'backbone.0.body.layer4.2.conv3.weight',
         'input_proj.weight', 'input_proj.bias',
         'transformer.encoder.layers.0.self_attn.in_proj_weight', 'transformer.encoder.layers.0.self_attn.in_proj_bias',
         'transformer.encoder.layers.0.linear1.weight',
         'transformer.decoder.layers.1.multihead_attn.in_proj_weight',
         'transformer.decoder.layers.1.multihead_attn.out_proj.weight',
         'transformer.decoder.norm.weight', 'transformer.decoder.norm.bias',
         'query_embed.weight', 'class_embed.weight', 'class_embed.bias', 'bbox_embed.layers.2.weight')
LOSSES = ('loss_ce', 'loss_bbox', 'loss_giou', 'cardinality_error', 'class_error')
SETS = ('', '_0')                                        # final, the one auxiliary layer

N_TRACK, TRACK_SEED, TRACK_W_SEED = 5, 6113, 6114
TRACK_QSEL = tuple(range(0, 8)) + tuple(range(8, N_TRACK + 100, 8))   # the track queries, then every 8th


def gen(seed):
    return torch.Generator().manual_seed(seed)


def frames(dtype=torch.float32):
    return [torch.randn(3, h, w, generator=gen(s)).to(dtype) for s, h, w in FRAMES]


def targets(dtype=torch.float32):
    """Per frame: boxes with centres in (0.25, 0.75) and sides in (0.15, 0.45) of the frame, labels in [1, 90]."""
    out = []
    for seed, n in TARGETS:
        g = gen(seed)
        boxes = torch.cat([torch.rand(n, 2, generator=g) * 0.5 + 0.25, torch.rand(n, 2, generator=g) * 0.3 + 0.15], -1)
        out.append({'boxes': boxes.to(dtype), 'labels': torch.randint(1, 91, (n,), generator=g)})
    return out


def loss_keys():
    keys = []
    for s in SETS:
        keys += [k + s for k in LOSSES if not (k == 'class_error' and s)]
    return keys


def track_embeds(d, dtype=torch.float32):
    """N_TRACK track-query embeddings per frame, (frames, N_TRACK, d)."""
    return torch.randn(len(FRAMES), N_TRACK, d, generator=gen(TRACK_SEED)).to(dtype)


def track_weights(n_logits, dtype=torch.float32):
    """W1 (frames, N_TRACK + 100, n_logits), W2 (frames, N_TRACK + 100, 4) of the criterion-free loss
    sum(pred_logits * W1) + sum(pred_boxes * W2)."""
    g = gen(TRACK_W_SEED)
    q = N_TRACK + 100
    return (torch.randn(len(FRAMES), q, n_logits, generator=g).to(dtype),
            torch.randn(len(FRAMES), q, 4, generator=g).to(dtype))
