"""What the reference's train loop does to a batch between the loader and model(imgs), on the device:

    multi_scale_size / resize_batch / preprocess_batch   train.py:380 + 394-399: `imgs.float() / 255` and the --multi-scale resize as ONE launch of
                                                         y3_resize_bilinear (csrc/batch_edge.hip) on the uint8 batch -- no fp32 intermediate
    quad_collate                                         utils/dataloaders.py:833-858 (collate_fn4, --quad; train.py:288): one launch of y3_quad_collate_u8 for
                                                         the images, the reference's label arithmetic on the host

The random draws are the reference's, call for call: a seeded run resizes to the sizes the reference draws and leaves the generator where the reference leaves it.
The rest of the loader side (mosaic, random_perspective, HSV, mixup, flips, load_image) is not here."""
from __future__ import annotations

import math
import random

import torch

from . import ops


def multi_scale_size(shape_hw, imgsz: int, gs: int = 32, rng=random):
    """The size train.py:395-398 resizes a batch of spatial shape `shape_hw` to, or None where the reference leaves the batch alone (sf == 1).  One
    rng.randrange call, as there."""
    sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5) + gs) // gs * gs
    sf = sz / max(shape_hw)
    if sf == 1:
        return None
    h, w = (math.ceil(x * sf / gs) * gs for x in shape_hw)   # stretched to a gs-multiple
    return h, w


def resize_batch(imgs: torch.Tensor, size, dtype: torch.dtype | None = None) -> torch.Tensor:
    """F.interpolate(imgs, size=size, mode="bilinear", align_corners=False) of a device batch (n, c, h, w) in one launch.  A uint8 batch is divided by 255 first
    (train.py:380) and comes back as `dtype` (default float32); a floating batch is not divided and keeps its dtype unless `dtype` is given.  A same-size call
    on uint8 is exactly imgs.float() / 255."""
    u8 = imgs.dtype == torch.uint8
    return ops.resize_bilinear(imgs, size, out_dtype=dtype, div=255.0 if u8 else 1.0)


def preprocess_batch(imgs: torch.Tensor, imgsz: int, gs: int = 32, multi_scale: bool = False, dtype: torch.dtype = torch.float32, rng=random) -> torch.Tensor:
    """train.py:380 + 394-399 in one call: the loader's uint8 batch goes to the current device if it is not there yet, is divided by 255 and,
    with multi_scale, resized to the size the reference draws -- one kernel launch, the result in `dtype`.  Under autocast pass dtype=torch.float16: rounding the
    fp32 result to half here is what autocast's cast of the first convolution's input does in the reference."""
    if imgs.dtype != torch.uint8:
        raise TypeError(f"preprocess_batch expects the loader's uint8 batch, not {imgs.dtype} (resize_batch takes floating batches)")
    if not imgs.is_cuda:
        imgs = imgs.to("cuda", non_blocking=True)
    size = multi_scale_size(imgs.shape[2:], imgsz, gs, rng) if multi_scale else None
    return resize_batch(imgs, size if size is not None else imgs.shape[2:], dtype)


def quad_labels(targets: torch.Tensor, bs: int, flags) -> torch.Tensor:
    """The label half of collate_fn4 on the host: `targets` (n, 6) [image, class, x, y, w, h] grouped by image, flags[g] true where group g was upsampled.
    An upsampled group keeps image 4g's rows; a tiled group takes its four images' rows in order, +1 on y for 4g+1, +1 on x for 4g+2, both for 4g+3, then
    xywh * 0.5; the image index becomes g."""
    if len(flags) != bs // 4:
        raise ValueError(f"quad_labels: {len(flags)} flags for a batch of {bs}")
    image = targets[:, 0].long()
    group, place = image // 4, image % 4   # place in the 2x2 tile: 0 top left, 1 bottom left, 2 top right, 3 bottom right
    tiled = ~torch.tensor(list(flags), dtype=torch.bool)[group]
    out = targets.clone()   # the caller's tensor is left alone
    out[tiled & (place % 2 == 1), 3] += 1.0    # the lower images sit one image height down
    out[tiled & (place >= 2), 2] += 1.0        # the right ones one image width across
    out[tiled, 2:] *= 0.5                      # the tile is twice as wide and high as one image
    out[:, 0] = group
    return out[tiled | (place == 0)]           # an upsampled group shows its first image only


def quad_collate(imgs: torch.Tensor, targets: torch.Tensor, rng=random):
    """The reference's collate_fn4 (--quad) on a collated batch: `imgs` uint8 (bs, c, h, w) on the device, bs % 4 == 0; `targets` the loader's CPU (n, 6) tensor,
    grouped by image.  One `rng.random() < 0.5` draw per group of four, in group order, decides between the bilinear x2 upsample of the group's first image and
    the 2x2 tile of all four; the flags are uploaded and the images made in one launch, the labels rebuilt on the host with the reference's arithmetic.
    Returns (imgs4 uint8 (bs / 4, c, 2h, 2w) on the device, targets4 on the CPU).

    The caller keeps what collate_fn4 and train.py do besides: paths[:bs // 4], shapes[:bs // 4], and `loss *= 4` (train.py:407)."""
    ops.require_gpu(imgs, "quad_collate")
    if targets.is_cuda:
        raise TypeError("quad_collate expects the loader's CPU targets (train.py:404 moves them to the device after the collate)")
    if imgs.dim() != 4 or imgs.dtype != torch.uint8:
        raise TypeError("quad_collate expects a uint8 (bs, c, h, w) batch")
    if targets.dim() != 2 or targets.shape[1] != 6:
        raise TypeError("quad_collate expects (n, 6) targets [image, class, x, y, w, h]")
    bs = imgs.shape[0]
    if bs % 4:
        raise ValueError(f"quad_collate: batch size {bs} is not a multiple of 4")
    flags = [rng.random() < 0.5 for _ in range(bs // 4)]
    dflags = torch.tensor(flags, dtype=torch.uint8).to(imgs.device, non_blocking=True)
    return ops.quad_collate_u8(imgs, dflags), quad_labels(targets, bs, flags)
