"""GPU tests of the device-side batch preparation (csrc/batch_edge.hip through yolov3_amd/batching.py): y3_resize_bilinear against torch's CPU
F.interpolate of `u.float() / 255` computed here, y3_quad_collate_u8 against the outputs of the unmodified reference's collate_fn4
(tests/golden/batching.pt, made by tests/golden/make_batching_golden.py), and three --multi-scale training steps end to end."""
import random
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "batching.pt", weights_only=True)   # data only


def u8_batch(shape, seed=0):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# the smallest shapes that reach each path of the kernel
RESIZE_CASES = {
    "up": ((2, 3, 64, 96), (96, 160)),
    "down-non-integer-ratio": ((2, 3, 96, 160), (64, 96)),
    "source-width-off-the-vector-width": ((1, 3, 33, 70), (64, 128)),
    "scalar-tail-less-than-a-wave": ((1, 1, 5, 7), (3, 13)),
    "planes-beyond-the-grid": ((24, 3, 8, 8), (16, 16)),   # 72 planes, 64 at most in the grid: the stride loop runs
}


@pytest.mark.parametrize("case", list(RESIZE_CASES))
def test_resize_u8_to_fp32_matches_torch_cpu(case):
    """atol 2.5e-7, the tolerance test_scale_img_vs_reference_golden pins for this arithmetic against torch's CPU kernel (2 ulp of fp32 below 1)"""
    from yolov3_amd import resize_batch

    shape, size = RESIZE_CASES[case]
    u = u8_batch(shape)
    ref = F.interpolate(u.float() / 255, size=size, mode="bilinear", align_corners=False)
    got = resize_batch(u.to(DEV), size)
    assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_contiguous()
    print(case, "max abs err", (got.cpu() - ref).abs().max().item())
    torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=2.5e-7)


def test_resize_same_size_is_exactly_the_division_and_empty_batches_pass():
    from yolov3_amd import ops, preprocess_batch, resize_batch

    for shape in ((2, 3, 64, 96), (1, 1, 5, 7)):
        u = u8_batch(shape, seed=1)
        assert torch.equal(resize_batch(u.to(DEV), shape[2:]).cpu(), u.float() / 255)
        assert torch.equal(preprocess_batch(u, 640).cpu(), u.float() / 255)   # a CPU batch is moved; no multi_scale: no resize
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16)   # every byte value
    assert torch.equal(resize_batch(u.to(DEV), (16, 16)).cpu(), u.float() / 255)
    empty = resize_batch(torch.empty(0, 3, 64, 96, dtype=torch.uint8, device=DEV), (96, 160))
    assert empty.shape == (0, 3, 96, 160) and empty.dtype == torch.float32
    with pytest.raises(TypeError, match="float32 / float16 / bfloat16"):
        ops.resize_bilinear(u.to(DEV), (16, 16), out_dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.resize_bilinear(u.to(DEV).long(), (16, 16))


@pytest.mark.parametrize("src,dst", [(torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.uint8, torch.float16),
                                     (torch.uint8, torch.bfloat16), (torch.float16, torch.float32), (torch.float32, torch.bfloat16)], ids=str)
def test_resize_other_dtype_pairs(src, dst):
    """against the fp32 torch result rounded once to the output type: for values in [0, 1) at most one unit in the last place of fp16 (2^-10) / bf16 (2^-7), the
    bound test_scale_img_vs_reference_golden uses; fp32 output as above"""
    from yolov3_amd import ops, resize_batch

    bound = {torch.float32: 2.5e-7, torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}[dst]
    for shape, size in (((2, 3, 64, 96), (96, 160)), ((2, 3, 96, 160), (64, 96)), ((1, 1, 5, 7), (3, 13))):
        if src == torch.uint8:
            x = u8_batch(shape, seed=2)
            xf = x.float() / 255
        else:
            x = torch.rand(shape, generator=torch.Generator().manual_seed(2)).to(src)
            xf = x.float()
        ref = F.interpolate(xf, size=size, mode="bilinear", align_corners=False).to(dst)
        got = resize_batch(x.to(DEV), size, dtype=None if dst == src else dst)
        assert got.dtype == dst and got.shape == ref.shape
        err = (got.float().cpu() - ref.float()).abs().max().item()
        print(src, dst, shape, size, "max abs err", err)
        assert err <= bound, (src, dst, shape, size, err)
    # a divisor on a floating source (ops level): to_f32(x) / div, then the interpolate
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(3)).to(src if src != torch.uint8 else torch.float32)
    ref = F.interpolate(x.float() / 3.0, size=(16, 24), mode="bilinear", align_corners=False).to(dst)
    got = ops.resize_bilinear(x.to(DEV), (16, 24), out_dtype=dst, div=3.0)
    assert (got.float().cpu() - ref.float()).abs().max().item() <= bound


def test_resize_more_tiles_than_the_grid_holds():
    """one plane of 1040 x 4096: 2080 tiles of 32 segments against a grid of at most 2048 blocks, so the tile stride loop runs (and its barrier with it)"""
    from yolov3_amd import resize_batch

    u = u8_batch((1, 1, 3, 5), seed=6)
    ref = F.interpolate(u.float() / 255, size=(1040, 4096), mode="bilinear", align_corners=False)
    got = resize_batch(u.to(DEV), (1040, 4096))
    torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=2.5e-7)
    refh = ref.half()
    assert (resize_batch(u.to(DEV), (1040, 4096), dtype=torch.float16).float().cpu() - refh.float()).abs().max().item() <= 2.0**-10


def collated(labels):
    out = [lb.clone() for lb in labels]
    for i, lb in enumerate(out):
        lb[:, 0] = i
    return torch.cat(out, 0)


def test_quad_collate_matches_collate_fn4(gold):
    from yolov3_amd import quad_collate

    imgs, targets = gold["quad_in"]["imgs"], collated(gold["quad_in"]["labels"])
    assert imgs.shape == (8, 3, 6, 10)
    for seed, g in gold["quad"].items():   # [upsample, tile] and [tile, upsample]
        random.seed(seed)
        im4, lb4 = quad_collate(imgs.to(DEV), targets)
        assert random.random() == g["next_random"]
        assert im4.dtype == torch.uint8 and im4.is_cuda and not lb4.is_cuda
        assert torch.equal(im4.cpu(), g["imgs"]), (seed, g["flags"])
        assert torch.equal(lb4, g["labels"])
    with pytest.raises(TypeError, match="CPU targets"):
        quad_collate(imgs.to(DEV), targets.to(DEV))


def test_quad_collate_three_groups_mixed_flags(gold):
    from yolov3_amd import quad_collate

    g = gold["quad_big"]
    n = 12 * 3 * 32 * 40   # tests/golden/make_batching_golden.py::big_batch, pinned by the recorded sum
    big = (((torch.arange(n, dtype=torch.int64) * 1103515245 + 12345) >> 8) % 256).to(torch.uint8).reshape(12, 3, 32, 40)
    assert big.shape == (12, 3, 32, 40) and int(big.long().sum()) == g["input_sum"] and len(set(g["flags"])) == 2
    rng = random.Random(g["seed"])
    im4, lb4 = quad_collate(big.to(DEV), torch.zeros(0, 6), rng=rng)
    assert im4.shape == (3, 3, 64, 80) and lb4.shape == (0, 6)
    assert torch.equal(im4.cpu(), g["imgs"])


def test_quad_collate_odd_width_takes_the_byte_store_path():
    """a width the fixture does not hold (2w no multiple of 4: byte stores, a clamped last group), against collate_fn4's two torch expressions computed here"""
    from yolov3_amd import ops

    u = u8_batch((8, 2, 5, 7), seed=4)
    want = torch.stack([
        F.interpolate(u[0].unsqueeze(0).float(), scale_factor=2.0, mode="bilinear", align_corners=False)[0].to(torch.uint8),
        torch.cat((torch.cat((u[4], u[5]), 1), torch.cat((u[6], u[7]), 1)), 2)])
    got = ops.quad_collate_u8(u.to(DEV), torch.tensor([1, 0], dtype=torch.uint8, device=DEV))
    assert torch.equal(got.cpu(), want)


def test_quad_collate_more_items_than_the_grid_holds():
    """planes of 1040 x 2020: 525 200 four-byte groups against a grid of at most 2048 x 256 lanes, so the item stride loop runs; both branches, against
    collate_fn4's two torch expressions computed here"""
    from yolov3_amd import ops

    u = u8_batch((8, 1, 520, 1010), seed=7)
    want = torch.stack([
        torch.cat((torch.cat((u[0], u[1]), 1), torch.cat((u[2], u[3]), 1)), 2),
        F.interpolate(u[4].unsqueeze(0).float(), scale_factor=2.0, mode="bilinear", align_corners=False)[0].to(torch.uint8)])
    got = ops.quad_collate_u8(u.to(DEV), torch.tensor([0, 1], dtype=torch.uint8, device=DEV))
    assert torch.equal(got.cpu(), want)


def test_multi_scale_training_steps_end_to_end(gold):
    """yolov3-tiny, fp32, batch 2, uint8 128 x 128 batches, seeded `random`: three preprocess_batch(multi_scale=True) -> model -> ComputeLoss -> backward steps.
    The shapes that reach the engine are the fixture's; each loss agrees within 1e-4 relative (the bound the fp32 engine is held to against the reference goldens)
    with the same step fed torch's CPU resize of the same batch; the second pass over the same sizes builds no plan."""
    import yaml

    from oracle import yolo_oracle as yo
    from yolov3_amd import ComputeLoss, DetectionModel, preprocess_batch, train_engine

    name, nc, seed, imgsz, gs, bs = "yolov3-tiny", 80, 1, 128, 32, 2
    d = yaml.safe_load(open(ROOT / "yolov3_amd" / "cfg" / f"{name}.yaml"))
    layers, save, anchors, nc_v = yo.parse_cfg(d, 3, nc)
    sd = yo.seeded_state_dict(layers, nc_v, anchors, yo.model_strides(layers), seed=41)
    m = DetectionModel(f"{name}.yaml", nc=nc)
    m.load_state_dict(sd)
    m = m.to(DEV).float().train()
    m.hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
    crit = ComputeLoss(m)
    tg = yo.synth_targets(bs, nc, seed=5).to(DEV)
    batches = [u8_batch((bs, 3, imgsz, imgsz), seed=10 + i) for i in range(3)]
    want_sizes = gold["draws"][(seed, imgsz, (imgsz, imgsz))]["sizes"][:3]
    assert want_sizes == [[96, 96], [192, 192], [64, 64]]

    def step(x):
        m.zero_grad(set_to_none=True)
        loss, _ = crit(m(x), tg)
        loss.backward()
        return loss.item()

    random.seed(seed)
    fused, shapes = [], []
    for u in batches:
        x = preprocess_batch(u, imgsz, gs, multi_scale=True)
        assert x.dtype == torch.float32 and x.is_cuda
        shapes.append(list(x.shape[2:]))
        fused.append(step(x))
    assert shapes == want_sizes
    torch.cuda.synchronize()
    builds = train_engine.PLAN_BUILDS
    for u, size, a in zip(batches, shapes, fused):
        b = step(F.interpolate(u.float() / 255, size=size, mode="bilinear", align_corners=False).to(DEV))
        print(size, "loss fused", a, "torch-cpu resize", b, "rel", abs(a - b) / abs(b))
        assert abs(a - b) <= 1e-4 * abs(b), (size, a, b)
    assert train_engine.PLAN_BUILDS == builds, f"{train_engine.PLAN_BUILDS - builds} plans were built in the second pass over the same sizes"
    # under autocast the caller asks for half: the fp32 result rounded once
    random.seed(seed)
    xh = preprocess_batch(batches[0], imgsz, gs, multi_scale=True, dtype=torch.float16)
    ref = F.interpolate(batches[0].float() / 255, size=shapes[0], mode="bilinear", align_corners=False).half()
    assert xh.dtype == torch.float16 and (xh.float().cpu() - ref.float()).abs().max().item() <= 2.0**-10
