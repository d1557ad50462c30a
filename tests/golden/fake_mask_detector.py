"""FakeDetector (fake_detector.py) with segmentation masks, for the tracker-masks fixture
(tests/golden/make_golden_mots.py, tests/test_mots_gpu.py): pred_masks (1, K+Q, 24, 34), one row
per output row -- a bump of amplitude 3..7 at that row's OUTPUT box (radius 0.9 * box + 0.05 of the
image) minus 2.5 plus 0.3 * noise, clamped to |logit| <= 7.5 (f32 sigmoid saturates to exactly 1.0
near 16.7, and saturated ties would make the fixture ambiguous).  Amplitudes and noise come from a
SEPARATE CPU generator seeded by (mask_seed, seed, frame): boxes, logits and embeddings stay those
of FakeDetector, so the box bookkeeping is the one tracker.npz pins.

Blobs: original size 120x176, network-input size 96x136 (the masks' 24x34 is its stride 4); both
resize ratios (96 -> 24x4, 120 / 96, 176 / 136) are non-integer where it matters."""
import torch

from fake_detector import FakeDetector, sequence_blobs

MASK_HW = (24, 34)
NET_HW = (96, 136)
ORIG_HW = (120, 176)
MASK_SEED = 0        # make_golden_mots.py searches from here; the fixture stores the one it took


class FakeMaskDetector(FakeDetector):
    def __init__(self, mask_seed=MASK_SEED, **kw):
        super().__init__(**kw)
        self.mask_seed = mask_seed

    def forward(self, img, targets=None, prev_features=None):
        frame = self.frame
        out, *rest = super().forward(img, targets, prev_features)
        g = torch.Generator().manual_seed(7_000_000 + self.mask_seed * 100_000 + self.seed * 1000 + frame)
        boxes = out['pred_boxes'][0].detach().cpu().float()            # (K+Q, 4) cxcywh in [0, 1]
        n = boxes.shape[0]
        H, W = MASK_HW
        ys = ((torch.arange(H, dtype=torch.float32) + 0.5) / H).view(1, H, 1)
        xs = ((torch.arange(W, dtype=torch.float32) + 0.5) / W).view(1, 1, W)
        cx, cy, bw, bh = (boxes[:, i].view(n, 1, 1) for i in range(4))
        r2 = ((xs - cx) / (0.9 * bw + 0.05)) ** 2 + ((ys - cy) / (0.9 * bh + 0.05)) ** 2
        amp = torch.rand(n, 1, 1, generator=g) * 4.0 + 3.0
        masks = amp * torch.exp(-r2) - 2.5 + 0.3 * torch.randn(n, H, W, generator=g)
        out['pred_masks'] = masks.clamp(-7.5, 7.5)[None].to(self.anchor.device)
        return (out, *rest)


def mask_blobs(seed, frames, device='cpu'):
    """sequence_blobs at the fixture's original size, plus the network-input size the tracker passes
    to PostProcessSegm as max_target_sizes (tracker.py:322)."""
    blobs = sequence_blobs(seed, frames, size=ORIG_HW, device=device)
    for b in blobs:
        b['size'] = torch.tensor([list(NET_HW)], device=device)
    return blobs
