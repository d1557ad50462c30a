"""`build_model(args) -> (model, criterion, postprocessors)`, mirroring
src/trackformer/models/__init__.py:16-125.

    from kinet_amd.models import build_model      # instead of trackformer.models
    model, criterion, postprocessors = build_model(args)
    model.set_compute_dtype(torch.bfloat16)        # optional perf mode (default fp32)

`args` is the reference's Namespace (cfgs/train.yaml + named configs).  All three model
families are built: the deformable image branch (:51-71, the hot path), the KineT kinematic
branch (`args.kine`, :72-107, kinet_amd/models/kinet.py) and vanilla DETR (:111-125, the
reference's default `deformable: false`; kinet_amd/models/detr.py, inference and f32 training).  The
deformable branch also builds the two-stage variant (`two_stage: true`; the proposal stage runs on
csrc/two_stage.hip; what build_model returns is the inference model, and training it is opt-in:
kinet_amd.train.build_two_stage_training(args) returns the same model with `two_stage_training` set
and the criterion rebuilt with build_criterion(..., enc_losses=True), csrc/criterion.hip) and, with `masks: true` (cfgs/train_coco_person_masks.yaml,
cfgs/train_mots20.yaml), DeformableDETRSegm / DeformableDETRSegmTracking plus the 'segm'
postprocessor (:63-69, :165-166; kinet_amd/models/segmentation.py on csrc/segm.hip:
`out['pred_masks']`).  What build_model returns for masks is the inference model: under autograd
it raises, and its criterion carries no mask / dice losses.  Training the mask head is opt-in:
kinet_amd.train.build_mask_training(args) returns the same model with `mask_training` set and the
criterion rebuilt with build_criterion(..., mask_losses=True) (csrc/segm_train.hip).  Still
raising NotImplementedError: `masks` without `deformable` (vanilla DETRSegm / DETRSegmTracking) or
with `two_stage`, and the panoptic postprocessor (dataset coco_panoptic).
"""
import torch

from kinet_amd.models.backbone import build_backbone
from kinet_amd.models.deformable_detr import DeformableDETR, DeformablePostProcess, PostProcess
from kinet_amd.models.deformable_transformer import build_deforamble_transformer
from kinet_amd.models.detr import DETR
from kinet_amd.models.detr_tracking import DeformableDETRTracking, DETRTracking
from kinet_amd.models.segmentation import DeformableDETRSegm, DeformableDETRSegmTracking, PostProcessSegm
from kinet_amd.models.misc import NestedTensor, NestedTensorKinet, nested_tensor_from_tensor_list

NUM_CLASSES = {'coco': 91, 'coco_panoptic': 250, 'coco_person': 20, 'mot': 20, 'mot_crowdhuman': 20,
               'crowdhuman': 20, 'mot_coco_person': 20, 'mot_kine': 1}


def build_model(args):
    if args.dataset not in NUM_CLASSES:
        raise NotImplementedError(args.dataset)
    num_classes = NUM_CLASSES[args.dataset]
    if getattr(args, 'kine', False) and not args.deformable:
        from kinet_amd.models.criterion import build_criterion
        from kinet_amd.models.kinet import build_kinet
        from kinet_amd.models.matcher import build_matcher
        matcher = build_matcher(args)
        model = build_kinet(args, num_classes)
        post = {'bbox': DeformablePostProcess() if args.focal_loss else PostProcess()}
        return model, build_criterion(args, num_classes, matcher), post
    masks = bool(getattr(args, 'masks', False))
    if masks and not args.deformable:
        raise NotImplementedError('segmentation heads are built for Deformable DETR only: vanilla DETRSegm / '
                                  'DETRSegmTracking (masks without deformable) are not built')
    if masks and args.two_stage:
        raise NotImplementedError('masks with two_stage is not built')
    if masks and args.dataset == 'coco_panoptic':
        raise NotImplementedError('PostProcessPanoptic is not built')
    if not args.deformable:
        return _build_detr(args, num_classes)
    if args.two_stage and (args.tracking or args.multi_frame_attention):
        # the reference's two-stage branch builds its queries from the proposals alone and drops
        # the track queries (deformable_transformer.py:180-194)
        raise NotImplementedError('two_stage with tracking / multi_frame_attention is not built: the two-stage '
                                  'branch of the reference ignores track queries')
    backbone = build_backbone(args)
    matcher = None
    try:
        from kinet_amd.models.matcher import build_matcher
        matcher = build_matcher(args)
    except ImportError:
        pass
    detr_kwargs = {
        'backbone': backbone,
        'num_classes': num_classes - 1 if args.focal_loss else num_classes,
        'num_queries': args.num_queries,
        'aux_loss': args.aux_loss,
        'overflow_boxes': args.overflow_boxes,
        'transformer': build_deforamble_transformer(args),
        'num_feature_levels': args.num_feature_levels,
        'with_box_refine': args.with_box_refine,
        'two_stage': args.two_stage,
        'multi_frame_attention': args.multi_frame_attention,
        'multi_frame_encoding': args.multi_frame_encoding,
        'merge_frame_features': args.merge_frame_features,
    }
    mask_kwargs = {'freeze_detr': getattr(args, 'freeze_detr', False)}
    if args.tracking:
        tracking_kwargs = {
            'track_query_false_positive_prob': args.track_query_false_positive_prob,
            'track_query_false_negative_prob': args.track_query_false_negative_prob,
            'matcher': matcher,
            'backprop_prev_frame': args.track_backprop_prev_frame}
        if masks:
            model = DeformableDETRSegmTracking(mask_kwargs, tracking_kwargs, detr_kwargs)
        else:
            model = DeformableDETRTracking(tracking_kwargs, detr_kwargs)
    elif masks:
        model = DeformableDETRSegm(mask_kwargs, detr_kwargs)
    else:
        model = DeformableDETR(**detr_kwargs)
    criterion = None
    try:
        from kinet_amd.models.criterion import build_criterion
        criterion = build_criterion(args, num_classes, matcher)
    except ImportError:
        pass
    postprocessors = {'bbox': DeformablePostProcess()}
    if masks:
        # the criterion above carries no mask / dice losses: kinet_amd.train.build_mask_training adds them
        postprocessors['segm'] = PostProcessSegm()
    return model, criterion, postprocessors


def _build_detr(args, num_classes):
    """models/__init__.py:111-125: vanilla DETR (config 1).  As there, multi_frame_* are not
    passed on to the model."""
    from kinet_amd.models.criterion import build_criterion
    from kinet_amd.models.matcher import build_matcher
    from kinet_amd.models.transformer import build_transformer
    matcher = build_matcher(args)
    detr_kwargs = {
        'backbone': build_backbone(args),
        'num_classes': num_classes - 1 if args.focal_loss else num_classes,
        'num_queries': args.num_queries,
        'aux_loss': args.aux_loss,
        'overflow_boxes': args.overflow_boxes,
        'transformer': build_transformer(args),
    }
    if args.tracking:
        tracking_kwargs = {
            'track_query_false_positive_prob': args.track_query_false_positive_prob,
            'track_query_false_negative_prob': args.track_query_false_negative_prob,
            'matcher': matcher,
            'backprop_prev_frame': args.track_backprop_prev_frame}
        model = DETRTracking(tracking_kwargs, detr_kwargs)
    else:
        model = DETR(**detr_kwargs)
    post = {'bbox': DeformablePostProcess() if args.focal_loss else PostProcess()}
    return model, build_criterion(args, num_classes, matcher), post


__all__ = ['build_model', 'DETR', 'DETRTracking', 'DeformableDETR', 'DeformableDETRTracking', 'DeformablePostProcess', 'PostProcess',
           'DeformableDETRSegm', 'DeformableDETRSegmTracking', 'PostProcessSegm',
           'NestedTensor', 'NestedTensorKinet', 'nested_tensor_from_tensor_list']
