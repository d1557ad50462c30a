"""Conditioning of the name-seeded weights (weights.py) for the segmentation fixtures, shared by
the generator (make_golden_segm.py, on the reference model) and the tests (on kinet_amd's).

With `randomize` alone the reference's masks do not depend on the query: the attention map is
near-uniform and the FPN adapters swamp the query path, so max_q - min_q of pred_masks is 0.0000
at every pixel, and a fixture like that passes with a broken attention map or a wrong query
order.  After `condition` the median spread over the queries is >= 0.5 (make_golden_segm.py
asserts >= 0.1 per frame).
"""
import torch

LAY1_ATT_GAIN = 64.0     # mask_head.lay1.weight[:, hidden_dim:], the attention channels
QK_GAIN = 4.0            # bbox_attention.{q,k}_linear.weight
ADAPTER_GAIN = 0.1       # mask_head.adapter{1,2,3}.{weight,bias}


def randomize_segm(model, seed):
    """weights.randomize + condition; returns the model."""
    from weights import randomize
    randomize(model, seed=seed)
    return condition(model)


@torch.no_grad()
def condition(model):
    head, att = model.mask_head, model.bbox_attention
    head.lay1.weight[:, att.hidden_dim:] *= LAY1_ATT_GAIN
    att.q_linear.weight *= QK_GAIN
    att.k_linear.weight *= QK_GAIN
    for ad in (head.adapter1, head.adapter2, head.adapter3):
        ad.weight *= ADAPTER_GAIN
        ad.bias *= ADAPTER_GAIN
    return model
