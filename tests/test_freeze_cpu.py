"""Frozen-layer training, host side (no GPU): freeze_layers against the reference's own loop (train.py:217-223, restated below), the training plan's need analysis
(which backward passes a plan runs for a requires_grad pattern), the gradient arena's size, the plan cache's key and the packing schedule of frozen filter banks."""
import pytest
import torch

from yolov3_amd import DetectionModel, freeze_layers, ops
from yolov3_amd.train_engine import Act, ConvUnit, HeadUnit, TrainPlan, TrainSlot, acquire_plan, need_pattern

CPU = torch.device("cpu")


def reference_freeze(model, freeze):
    """reference train.py:217-223, verbatim but for the logger"""
    freeze = [f"model.{x}." for x in (freeze if len(freeze) > 1 else range(freeze[0]))]  # layers to freeze
    for k, v in model.named_parameters():
        v.requires_grad = True  # train all layers
        if any(x in k for x in freeze):
            v.requires_grad = False
    return {k for k, v in model.named_parameters() if not v.requires_grad}


def layer_of(u):
    return int(u.label[1:].split(".")[0]) if isinstance(u, ConvUnit) else -1


def plan_for(name, freeze, dtype=torch.float16):
    m = DetectionModel(f"{name}.yaml", nc=80).train()
    freeze_layers(m, freeze)
    return m, TrainPlan.build(m, 2, 64, 64, dtype, CPU, TrainSlot(dtype, CPU))


@pytest.mark.parametrize("freeze", [[0], [10], [1], [0, 1, 2]])
@pytest.mark.parametrize("name", ["yolov3", "yolov3-tiny"])
def test_freeze_layers_matches_the_reference_loop(name, freeze):
    m = DetectionModel(f"{name}.yaml", nc=80)
    for p in list(m.parameters())[::3]:
        p.requires_grad = False   # (whatever was set before is overwritten: "train all layers")
    want = reference_freeze(m, freeze)
    for p in m.parameters():
        p.requires_grad = True
    got = freeze_layers(m, freeze)
    assert set(got) == want and len(got) == len(want)
    assert {k for k, v in m.named_parameters() if not v.requires_grad} == want
    if freeze == [0]:
        assert got == []
    if freeze == [0, 1, 2]:   # substring matching, as upstream: the dot behind the index keeps model.1. out of model.11. / model.21. (their names hold "model.11.", not "model.1.")
        assert {k.split(".")[1] for k in got} == ({"0", "1", "2"} if name == "yolov3" else {"0", "2"})   # (layer 1 of yolov3-tiny is a MaxPool2d)
    if freeze == [1]:
        assert got and all(k.startswith("model.0.") for k in got)


def test_backbone_freeze_of_yolov3_has_no_backward_work_below_layer_10():
    m, p = plan_for("yolov3", [10])
    convs = [u for u in p.units if isinstance(u, ConvUnit)]
    assert len(convs) == 72
    below = [u for u in convs if layer_of(u) < 10]
    assert len(below) == 44
    for u in below:
        assert not (u.active or u.wgrad_on or u.dgamma_on or u.dbeta_on or u.need_dx or u.need_res or u.pair_pack), u.label
        assert not u.y.need and not u.x.need and u.bank_dgrad is None and (u.use_stem or u.bank_fwd is not None)
    first = next(u for u in convs if layer_of(u) == 10)
    assert first.label == "L10.0.cv1" and first.active and first.wgrad_on and first.dgamma_on and first.dbeta_on and not first.need_dx and first.bank_dgrad is None
    second = convs[convs.index(first) + 1]
    assert second.label == "L10.0.cv2" and second.res is first.x and second.need_dx and not second.need_res, "the shortcut of the first live Bottleneck: its input needs no gradient"
    for u in convs[convs.index(second):]:
        assert u.active and u.wgrad_on and u.need_dx, u.label
        assert u.need_res == (u.res is not None and u is not second)
    assert all(hd.w_on and hd.b_on and hd.need_dx for hd in p.heads)
    # layers 6 and 8 sit in slices of the Concat buffers of layers 25 and 18: the buffers' gradients exist (the upsampled branch needs its slice), theirs are not asked for
    cats = [a for a in p.acts if a.slices]
    assert len(cats) == 2 and all(a.need for a in cats) and sorted(s.need for a in cats for s in a.slices) == [False, False, True, True]
    with pytest.raises(RuntimeError, match="needs none"):
        below[-1].y.grad()
    with pytest.raises(RuntimeError, match="needs none"):
        p.x_in.grad()
    # the gradient arena holds the live parameters only (64-element slices, TrainPlan.grad_alloc), the exchange counts their bytes
    live = [q for q in m.parameters() if q.requires_grad]
    assert 0 < len(live) < len(p.params)
    assert p._arena_numel == sum((q.numel() + 63) // 64 * 64 for q in live)
    assert p.live_bytes == 4 * sum(q.numel() for q in live)
    assert p.live == need_pattern(m.parameters()) and sum(p.live) == len(live)


def test_every_parameter_live_marks_what_the_engine_always_ran():
    for name in ("yolov3", "yolov3-tiny", "yolov3-spp"):
        m, p = plan_for(name, [0])
        assert all(a.need for a in p.acts) and not p.x_in.need
        for i, u in enumerate(p.units):
            if isinstance(u, ConvUnit):
                assert u.active and u.wgrad_on and u.dgamma_on and u.dbeta_on and u.need_dx == (i > 0) and u.need_res == (u.res is not None)
        assert p._arena_numel == sum((q.numel() + 63) // 64 * 64 for q in m.parameters())
        assert all(always for _, always in p.pack_select) and [j for j, _ in p.pack_select] == list(range(len(p.pack_jobs.jobs)))


def test_freezing_one_middle_stage_keeps_every_data_gradient():
    _, full = plan_for("yolov3", [0])
    m, p = plan_for("yolov3", [4, 4])   # (a list of more than one element names layers: layer 4 alone)
    assert {k.split(".")[1] for k, v in m.named_parameters() if not v.requires_grad} == {"4"}
    for u, v in zip(p.units, full.units):
        if not isinstance(u, ConvUnit):
            assert u.x.need and u.y.need
            continue
        assert u.label == v.label and u.active and u.need_dx == v.need_dx and u.need_res == v.need_res and u.pair_pack == v.pair_pack
        frozen = layer_of(u) == 4
        assert u.wgrad_on == u.dgamma_on == u.dbeta_on == (not frozen), u.label
    assert sum(1 for u in p.units if isinstance(u, ConvUnit) and not u.wgrad_on) == 4 and all(a.need for a in p.acts)


def test_head_side_freeze_and_pools():
    """yolov3 [27] (a list of one layer index is written twice: [27] alone would mean range(27)): the last neck block is frozen, its input still needs a gradient.
    yolov3-tiny [5] and yolov3-spp [10]: pooling / SPP units under a frozen prefix have nothing to do, those behind a live layer run."""
    _, p = plan_for("yolov3", [27, 27])
    l27 = [u for u in p.units if layer_of(u) == 27]
    assert len(l27) == 4 and all(u.active and u.need_dx and not (u.wgrad_on or u.dgamma_on or u.dbeta_on) for u in l27)
    assert all(u.wgrad_on for u in p.units if isinstance(u, ConvUnit) and layer_of(u) != 27)
    _, t = plan_for("yolov3-tiny", [5])
    kinds = [(type(u).__name__, u.x.need) for u in t.units if not isinstance(u, ConvUnit)]
    assert kinds == [("MaxPoolUnit", False)] * 3 + [("MaxPoolUnit", True)] * 3 + [("UpsampleUnit", True)], kinds   # layers 1, 3, 5 | 7, 9, 11 + 12 | 17
    assert [u.active for u in t.units if isinstance(u, ConvUnit)][:4] == [False, False, False, True]      # layers 0, 2, 4 | 6: behind the frozen pool, no data gradient
    conv6 = [u for u in t.units if isinstance(u, ConvUnit)][3]
    assert conv6.wgrad_on and not conv6.need_dx
    _, s = plan_for("yolov3-spp", [10])
    spp = next(u for u in s.units if type(u).__name__ == "SPPPoolUnit")
    assert spp.x.need and spp.y.need
    m2 = DetectionModel("yolov3-spp.yaml", nc=80).train()
    for k, v in m2.named_parameters():
        v.requires_grad = k.startswith("model.28.")   # only the Detect layer trains: nothing in front of the heads runs
    s2 = TrainPlan.build(m2, 2, 64, 64, torch.float16, CPU, TrainSlot(torch.float16, CPU))
    assert not any(u.active if isinstance(u, ConvUnit) else u.x.need for u in s2.units) and not any(a.need for a in s2.acts)
    assert all(hd.w_on and hd.b_on and not hd.need_dx and hd.bank_dgrad is None for hd in s2.heads)
    m2.model[28].m[0].weight.requires_grad = False   # weight and bias of a head are judged each on its own
    s3 = TrainPlan.build(m2, 2, 64, 64, torch.float16, CPU, TrainSlot(torch.float16, CPU))
    assert (s3.heads[0].w_on, s3.heads[0].b_on, s3.heads[1].w_on) == (False, True, True)


def test_bn_parameter_live_under_a_frozen_filter_still_gets_its_sums():
    """a pattern freeze_layers never makes: only one BatchNorm weight of the backbone trains.  Its unit runs the BatchNorm backward (dgamma is an output of it) but no
    filter gradient, no data gradient; every unit behind it passes the gradient on"""
    m = DetectionModel("yolov3-tiny.yaml", nc=80).train()
    for k, v in m.named_parameters():
        v.requires_grad = k == "model.4.bn.weight"
    p = TrainPlan.build(m, 2, 64, 64, torch.float32, CPU, TrainSlot(torch.float32, CPU))
    convs = [u for u in p.units if isinstance(u, ConvUnit)]
    u4 = next(u for u in convs if u.label == "L4")
    assert u4.active and u4.dgamma_on and not (u4.wgrad_on or u4.dbeta_on or u4.need_dx)
    assert [u.active for u in convs[:2]] == [False, False]
    assert all(u.active and u.need_dx and not u.wgrad_on for u in convs[convs.index(u4) + 1:])
    assert p._arena_numel == 64 and p.live_bytes == 4 * 64


def test_plan_cache_keys_on_the_requires_grad_pattern():
    m = DetectionModel("yolov3-tiny.yaml", nc=80).train()
    a = acquire_plan(m, 2, 64, 64, torch.float16, CPU, grad=False)
    assert acquire_plan(m, 2, 64, 64, torch.float16, CPU, grad=False) is a
    freeze_layers(m, [5])
    b = acquire_plan(m, 2, 64, 64, torch.float16, CPU, grad=False)
    assert b is not a and b.live != a.live and b.slot is a.slot
    assert acquire_plan(m, 2, 64, 64, torch.float16, CPU, grad=False) is b
    freeze_layers(m, [0])   # thaw: the first plan again, not a rebuild
    assert acquire_plan(m, 2, 64, 64, torch.float16, CPU, grad=False) is a
    next(m.parameters()).requires_grad = False
    c = acquire_plan(m, 2, 64, 64, torch.float16, CPU, grad=False)
    assert c is not a and c is not b and not c.units[0].wgrad_on and c.units[0].dgamma_on


def test_frozen_banks_are_packed_once_and_again_when_the_weight_version_moves():
    """the schedule of ops.PackJobs.run(select) (host logic; the launch itself is a GPU test): a live weight is packed at every forward, a frozen one when its banks
    do not hold the tensor's current (data_ptr, _version)"""
    m, p = plan_for("yolov3", [10])
    jobs, sel = p.pack_jobs, p.pack_select
    assert len(sel) == 71 + 3 and sum(1 for _, always in sel if not always) == 43   # (layer 0 packs its own stem bank)
    assert sum(1 for j in jobs.jobs if j[2] is not None) == 66 + 3 - 38 - 1        # no data-gradient bank under the frozen prefix (38 units + L10.0.cv1; layer 0 and the 5 stride-2 units never had one)
    assert jobs.stale(sel) == tuple(j for j, _ in sel)                              # nothing packed yet: all of them
    frozen = [j for j, always in sel if not always]
    for j in frozen:   # what run() notes after the launch
        w = jobs.jobs[j][0]
        jobs._packed[j] = (w.data_ptr(), w._version)
    assert jobs.stale(sel) == tuple(j for j, always in sel if always)
    w = jobs.jobs[frozen[3]][0]
    with torch.no_grad():
        w.copy_(torch.zeros_like(w))   # what load_state_dict does
    assert jobs.stale(sel) == tuple(j for j, always in sel if always or j == frozen[3])
    assert jobs.stale(None) == tuple(range(len(jobs.jobs)))
    # a second plan of the slot with every layer live registers its own jobs for the weights whose banks differ, and packs only its own
    freeze_layers(m, [0])
    q = TrainPlan.build(m, 2, 64, 64, torch.float16, CPU, p.slot, siblings=[p])
    assert all(always for _, always in q.pack_select) and len(q.pack_select) == 74 and len(jobs.jobs) == 74 + 39
    assert q.units[-1].bank_fwd is p.units[-1].bank_fwd and q.units[2].bank_fwd is not p.units[2].bank_fwd and q.units[1].bank_fwd is p.units[1].bank_fwd   # (the stride-2 layer 1 never had a data-gradient bank: one job)


def test_act_of_its_own_needs_a_gradient():
    """an Act made outside a plan (tools, the deferred-shortcut test) behaves as before: it may hold a gradient"""
    v = ops.View(torch.zeros(2 * 4 * 4 * 16, dtype=torch.float16), 2, 4, 4, 16, 16, 0)
    a = Act(v)
    assert a.need and a.grad().c == 16 and a.slice(0, 8).need
    assert isinstance(HeadUnit, type)
