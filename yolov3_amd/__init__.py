"""yolov3_amd -- MI355X-native (gfx950) implementation of the ultralytics/yolov3 detection hot path.

Public surface mirrors the reference's own Python signatures:
    DetectionModel / Model / Detect      (reference models/yolo.py)
    Conv / Bottleneck / SPP / Concat     (reference models/common.py)
    non_max_suppression, scale_boxes     (reference utils/general.py; + batched forms)
    process_batch                        (reference val.py:147-188; + batched form)
    ap_per_class / compute_ap / fitness  (reference utils/metrics.py:15-118; host NumPy, as in the reference)
    ap_per_class_device / ValStats / ConfusionMatrix / run_batches   (the same statistics kept and computed on the device: val.py:386-428)
    save_one_txt / save_one_json / output_to_target / coco80_to_coco91_class   (reference val.py:60-144, utils/plots.py:69-78, utils/general.py; + save_txt_batched /
                                         save_json_batched: the boxes of a batch converted by one launch, one copy to the host; run_batches(save_txt=, save_json=))
    CocoGroundTruth / CocoEval / CocoResult   (reference val.py:464-477: pycocotools' bbox AP / AR of the COCO-JSON, matched and accumulated on the device, bit for bit;
                                         run_batches(save_json=True, anno_json=...) puts its map / map50 into the results)
    ComputeLoss                          (reference utils/loss.py)
    FusedSGD / GradScaler / ModelEMA     (reference train.py:345,411-422: scaler.scale / unscale_ / clip / step / update / ema.update; ema.ema is the averaged model)
    smart_optimizer / FusedAdam / FusedAdamW / FusedRMSProp   (reference utils/torch_utils.py:207-237, train.py --optimizer; torch-format state dicts)
    check_anchors / kmean_anchors / anchor_metrics / check_anchor_order   (reference utils/autoanchor.py, train.py:255: metric, k-means and genetic loop on the device)
    labels_to_class_weights / labels_to_image_weights / image_weight_indices / LabelTable   (reference utils/general.py:543-568, train.py:333,360-363 --image-weights: the class
                                         histogram, the image weights and the weighted draw of the epoch's indices on the device; the host keeps the random stream)
    DeviceDataset / rect_batch_shapes    (reference utils/dataloaders.py:548-570, 659-735, 825-830; train.py:299-312, val.py:351-360: a cached augment=False dataset kept in device
                                         memory -- rect batch shapes on the host once, every letterboxed CHW RGB batch and its targets in one launch each, no host loader)
    DeviceTrainDataset / draw_item       (reference utils/dataloaders.py:659-735, 764-822; utils/augmentations.py:57-73, 137-216, 270-283: the augment=True loader -- mosaic, affine
                                         warp, HSV, flips and mixup sampled straight from the cached images in one launch per batch, the labels in another; the host keeps
                                         the reference's random stream; polygon labels (segments=) warp as 1000 resampled points per polygon in one more launch)
    DeviceRectTrainDataset               (reference utils/dataloaders.py:547-570, 659-735; utils/augmentations.py:104-216: the augment=True, rect=True loader of train.py --rect --
                                         the set in aspect-ratio order, every batch letterboxed to its own (H, W), affine warp, HSV and flips in the same two launches)
    store="host" on the three datasets   (the `--cache ram` cache where the reference keeps it: the images in pinned host memory, the images of the next batch staged into a
                                         small HBM ring by one launch on a side stream while the current step trains; the same batches bit for bit, for sets larger than HBM)
    multi_scale_size / resize_batch / preprocess_batch / quad_collate   (reference train.py:380,394-399 and utils/dataloaders.py:833-858 collate_fn4: the uint8 batch divided by 255 and
                                         resized for --multi-scale in one launch; the --quad collate in one launch)
    freeze_layers                        (reference train.py:217-223, --freeze: the training engine skips the backward work of frozen layers)
    save_checkpoint / smart_resume / strip_optimizer   (reference train.py:470-488, utils/torch_utils.py smart_resume, utils/general.py strip_optimizer)
    save_reference_checkpoint / export_reference / to_reference   (the way out: files the unmodified reference's attempt_load, strip_optimizer and smart_resume read)
    apply_classifier / apply_classifier_batched / classifier_crops / DeviceImages   (reference utils/general.py:827-859, detect.py:202-203: the second-stage classifier -- every
                                         detection of a batch cut out of its native image, resized to 224 x 224, RGB CHW / 255, in one launch; the rows the classifier confirms
                                         compacted in another)
    DetectMultiBackend (.pt branch), attempt_load, AutoShape   (reference models/common.py, models/experimental.py; Detections.crop())
    Ensemble                             (reference models/experimental.py:74-86, `--weights a.pt b.pt`: every member decodes into its window of one prediction)
Everything executes through libyolov3_hip.so (include/yolov3_hip.h); there is no CPU/PyTorch fallback.
"""
from .common import SPP, Bottleneck, Concat, Conv  # noqa: F401
from .general import non_max_suppression, non_max_suppression_batched, scale_boxes, scale_boxes_batched, xywh2xyxy, clip_boxes  # noqa: F401
from .val import detect_batches, process_batch, process_batch_batched, run_batches  # noqa: F401
from .metrics import ConfusionMatrix, ValStats, ap_per_class, ap_per_class_device, compute_ap, fitness  # noqa: F401
from .backend import DetectMultiBackend  # noqa: F401
from .autoanchor import anchor_metrics, check_anchor_order, check_anchors, kmean_anchors  # noqa: F401
from .label_weights import LabelTable, image_weight_indices, labels_to_class_weights, labels_to_image_weights  # noqa: F401
from .dataset import DeviceDataset, rect_batch_shapes  # noqa: F401
from .augment import DeviceRectTrainDataset, DeviceTrainDataset, draw_item  # noqa: F401
from .batching import multi_scale_size, preprocess_batch, quad_collate, resize_batch  # noqa: F401
from .autoshape import AutoShape, Detections, letterbox_batch  # noqa: F401
from .crops import DeviceImages, apply_classifier, apply_classifier_batched, classifier_crops  # noqa: F401
from .coco_eval import CocoEval, CocoGroundTruth, CocoResult  # noqa: F401
from .outputs import coco80_to_coco91_class, output_to_target, save_json_batched, save_one_json, save_one_txt, save_txt_batched  # noqa: F401
from .compat import attempt_load, save_checkpoint, smart_resume, strip_optimizer  # noqa: F401
from .compat import export_reference, reference_pickle_module, save_reference_checkpoint, to_reference  # noqa: F401
from .experimental import Ensemble  # noqa: F401
from .loss import ComputeLoss  # noqa: F401
from .optim import FusedAdam, FusedAdamW, FusedRMSProp, FusedSGD, GradScaler, ModelEMA, freeze_layers, smart_optimizer, smart_param_groups  # noqa: F401
from .yolo import Detect, DetectionModel, Model, parse_model  # noqa: F401

__version__ = "0.1.0"
