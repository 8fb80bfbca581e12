"""Sub-region classifier training on the GPU (isx_boxpool_s1_bwd_nhwc, isx/classif_head.py, TuneClassifSub's training hooks, the classifier
route of utils/train_general._Stepper): the box-pool backward against its canonical sum bit for bit and against float64 autograd, the engine tail
against float64, one optimizer step of TuneClassifSub(ResNet-50) on two scales against float64 autograd and against the torch-autograd tail, and
the entry point end to end."""
import copy
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


# ---- isx_boxpool_s1_bwd_nhwc ------------------------------------------------------------------------------------------------------------------
from _eval_model import boxpool_bwd_canonical as _canonical_boxpool_bwd


@pytest.mark.parametrize("B,H,W,kh,kw,C", [(2, 14, 14, 7, 7, 64), (1, 9, 11, 3, 5, 8), (3, 7, 7, 7, 7, 2048), (2, 6, 6, 1, 1, 4), (1, 10, 10, 7, 7, 260)])
def test_boxpool_backward_is_the_canonical_sum(B, H, W, kh, kw, C):
    from isx import ops
    Ho, Wo = H - kh + 1, W - kw + 1
    gen = torch.Generator().manual_seed(1000 * H + C)
    g = torch.randn(B, C, Ho, Wo, generator=gen)
    dx = ops.boxpool_s1_bwd_nhwc(g.cuda(), H, W, kh, kw)
    assert dx.shape == (B, C, H, W) and dx.permute(0, 2, 3, 1).is_contiguous()
    got = dx.cpu()
    want = torch.from_numpy(_canonical_boxpool_bwd(g.permute(0, 2, 3, 1).contiguous().numpy(), H, W, kh, kw)).permute(0, 3, 1, 2)
    assert torch.equal(got, want), float((got - want).abs().max())
    if (kh, kw) == (H, W):
        assert torch.equal(dx, ops.gap_bwd_nhwc(g.cuda().view(B, C), H, W))              # one term, the same division
    if (kh, kw) == (1, 1):
        assert torch.equal(got, g)
    for b in range(B):                                                                    # an image alone: the same bits as in the batch
        assert torch.equal(ops.boxpool_s1_bwd_nhwc(g[b:b + 1].cuda(), H, W, kh, kw), dx[b:b + 1])
    # arbiter: float64 autograd of F.avg_pool2d; e_cpu = the error of torch's own fp32 CPU autograd against it
    x64 = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    F.avg_pool2d(x64, (kh, kw), 1).backward(g.double())
    x32 = torch.zeros(B, C, H, W, requires_grad=True)
    F.avg_pool2d(x32, (kh, kw), 1).backward(g)
    ref = x64.grad
    e_gpu = float((got.double() - ref).abs().max())
    e_cpu = float((x32.grad.double() - ref).abs().max())
    print("box-pool backward %s: max |kernel - f64| = %.3g, max |torch CPU fp32 - f64| = %.3g" % ((B, H, W, kh, kw, C), e_gpu, e_cpu))
    floor = torch.from_numpy(4 * np.spacing(ref.abs().numpy().astype(np.float32)).astype(np.float64))
    over = (got.double() - ref).abs() > torch.clamp(floor, min=2 * e_cpu)
    assert not bool(over.any()), (e_gpu, e_cpu)


# ---- ClassifHeadEngine behind a box pool ------------------------------------------------------------------------------------------------------
def _bound(name, p):
    """The relative bounds tests/test_gpu_classif.py and tests/test_gpu_suffix.py assert for the same kinds of tensor: 2e-5 for weight matrices
    (convolution / Linear) and activations' gradients, 1e-5 for the small vectors (BatchNorm weight / bias, the classifier bias)."""
    return 2e-5 if p.dim() > 1 else 1e-5


def test_region_engine_tail_matches_float64_and_leaves_are_independent():
    from isx.classif_head import ClassifHeadEngine
    from model.siamese import BoxPool, PointwiseConv
    from test_gpu_suffix import _rel
    M, K, N, L = 4, 2048, 17, 4
    gen = torch.Generator().manual_seed(5)
    y_all = torch.randn(M, K, 9, 9, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, N, (M,), generator=gen).cuda()
    conv = PointwiseConv(K, N, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(N, K, 1, 1, generator=gen) * (7.0 / K ** 0.5))       # class scores of unit spread
        conv.bias.copy_(torch.randn(N, generator=gen) * 0.1)
    holder = types.SimpleNamespace(feature_reduc=nn.Sequential(BoxPool((7, 7), stride=1)), classifier=nn.Sequential(conv).cuda())
    assert ClassifHeadEngine.applicable(holder)
    eng = ClassifHeadEngine(holder)
    slices = {conv.weight: (0, N * K), conv.bias: (N * K, N * K + N)}
    scale_a, scale_b = 1.0 / 9, 0.125

    def run(y, lab, leaves):
        flat_all = torch.zeros(leaves, N * K + N, device="cuda")
        per_leaf, dy = eng.step(y, lab, leaves, scale_a, scale_b, flat_all, slices, need_dy=True)
        return per_leaf, dy, flat_all

    per_leaf, dy, flat_all = run(y_all, labels, L)
    assert dy.shape == y_all.shape and dy.permute(0, 2, 3, 1).is_contiguous()
    # gradients are ADDED into the leaves' rows
    again = flat_all.clone()
    eng.step(y_all, labels, L, scale_a, scale_b, again, slices, need_dy=False)
    assert torch.equal(again, flat_all + flat_all)
    y64 = y_all.double().requires_grad_(True)
    w64, b64 = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    for l in range(L):
        scores = F.conv2d(F.avg_pool2d(y64[l:l + 1], 7, 1), w64, b64)
        rows = scores.flatten(2).permute(0, 2, 1).reshape(-1, N)
        loss = F.cross_entropy(rows, labels[l:l + 1].expand(9), reduction="sum")
        gy, gw, gb = torch.autograd.grad(loss * (scale_a * scale_b), (y64, w64, b64))
        assert abs(float(per_leaf[l]) - float(loss)) <= 1e-5 * abs(float(loss)), (l, float(per_leaf[l]), float(loss))
        e_w = _rel(flat_all[l, :N * K].double().view(N, K), gw.view(N, K))
        e_b = _rel(flat_all[l, N * K:].double(), gb)
        e_y = _rel(dy[l].double(), gy[l])
        print("region engine leaf %d: loss %.7f (f64 %.7f), relative deviation weight %.3g, bias %.3g, dy %.3g" % (l, float(per_leaf[l]), float(loss), e_w, e_b, e_y))
        assert e_w <= 2e-5 and e_y <= 2e-5 and e_b <= 1e-5
        pl1, dy1, flat1 = run(y_all[l:l + 1], labels[l:l + 1], 1)                         # the leaf launched alone: the same bits
        assert torch.equal(pl1[0], per_leaf[l]) and torch.equal(dy1[0], dy[l]) and torch.equal(flat1[0], flat_all[l])


# ---- one optimizer step of TuneClassifSub(ResNet-50) on two scales ------------------------------------------------------------------------------
_CLASSES = 17


def _calibrated(classes, x):
    """TuneClassifSub(ResNet-50) with seeded weights whose BatchNorm running statistics are those of the images x (one training-mode pass) and
    whose classifier is scaled to class scores of unit spread (see tests/test_gpu_classif.py::_calibrated: gradients worth comparing need a
    net in its working range)."""
    from isx import backbones
    from model.siamese import TuneClassifSub
    from train.params import UNTRAINED_BLOCKS
    torch.manual_seed(0)
    net = TuneClassifSub(backbones.resnet50(pretrained=True, seed=0), classes, (7, 7), untrained=UNTRAINED_BLOCKS["resnet50"]).cuda()
    bns = [m for m in net.features.modules() if isinstance(m, nn.BatchNorm2d)]
    for m in bns:
        m.reset_running_stats()
        m.momentum = None                               # cumulative average: after one pass the running statistics ARE the batch's
    net.train()
    with torch.no_grad():
        net.features(x)
        for m in bns:
            m.momentum = 0.1
        net.eval()
        scores = net(x)[0]
        net.classifier[0].weight.div_(float(scores.std()) + 1e-12)
        net.classifier[0].bias.zero_()
    return net


@pytest.fixture(scope="module")
def setup():
    from model.nn_utils import set_net_train
    g = torch.Generator(device="cuda").manual_seed(7)
    x0 = torch.randn(4, 3, 288, 288, device="cuda", generator=g)
    x1 = F.interpolate(x0, size=(224, 224), mode="bicubic", align_corners=False)
    y = torch.randint(0, _CLASSES, (4,), device="cuda", generator=g)
    net = _calibrated(_CLASSES, x0)
    set_net_train(net, True, bn_train=False)
    return net, copy.deepcopy(net.state_dict()), (x0, x1), y


def _step(net, xs, y, batched=True):
    """One utils.train_general._Stepper step on 4 images at two scales, batch 4, micro-batch 1; returns (loss, {name: gradient})."""
    from model.custom_modules import CrossEntropyLoss
    from train import classif_regions as cr
    from train.params import Params
    from utils.train_general import _Stepper, make_sgd
    P = Params(cuda_device=0, train_batch_size=4, train_micro_batch=1, train_loss_avg=True, train_prefix_ahead=1, train_suffix_batched=batched)

    def create_batch(items, n):
        idx = torch.tensor(items, device="cuda")
        return [x[idx] for x in xs], [y[idx]]

    create_loss = cr.region_loss(CrossEntropyLoss(True), True)
    stepper = _Stepper(P, net, create_batch, create_loss)
    opt = make_sgd((p for p in net.parameters() if p.requires_grad), 1e-3, 0.0, 0.0)
    loss = stepper.step(opt, list(range(4)), {})
    torch.cuda.synchronize()
    return float(loss), dict((n, p.grad.detach().clone()) for n, p in net.named_parameters() if p.requires_grad)


def test_scales_step_matches_float64_autograd_and_the_autograd_tail(setup, monkeypatch):
    from model import nn_utils
    from model import siamese
    from test_gpu_suffix import _ref64_with_masks, _rel
    net, start, xs, y = setup
    net.load_state_dict(start)
    conv_calls = []
    hooks = [m.register_forward_hook(lambda m_, i_, o_: conv_calls.append(m_)) for m in net.features.modules() if isinstance(m, nn.Conv2d)]
    nn_utils.TORCH_CONV_CALLS.clear()
    loss, grads = _step(net, xs, y)
    for h in hooks:
        h.remove()
    assert nn_utils.TORCH_CONV_CALLS == {} and conv_calls == []              # no convolution of the step ran on torch / MIOpen
    assert net.classif_head_engine() is not None and net.suffix_engine() is not None
    after_on = copy.deepcopy(net.state_dict())
    # float64 autograd on the same prefix features with the engine's ReLU pattern pinned; the loss is the reference's formula
    net.load_state_dict(start)
    feats = net.precompute_trunk(*xs)
    assert [tuple(f.shape[2:]) for f in feats] == [(18, 18), (14, 14)]
    split = net._trunk.split
    eng = net.suffix_engine()
    blocks64 = copy.deepcopy(nn.Sequential(*list(net.features)[split:])).double()
    conv64 = copy.deepcopy(net.classifier[0]).double()
    loss64 = 0.0
    for f, loc in zip(feats, (9, 1)):
        _, saved = eng.forward(f)
        masks = [tuple((t > 0).permute(0, 3, 1, 2).double() for t in (t1, t2, yb)) for _, t1, t2, yb in saved]
        y64 = _ref64_with_masks(blocks64, f.double(), masks)
        scores = F.conv2d(F.avg_pool2d(y64, 7, 1), conv64.weight, conv64.bias)
        assert scores.shape[2] * scores.shape[3] == loc
        rows = scores.flatten(2).permute(0, 2, 1).reshape(-1, _CLASSES)
        per_image = F.cross_entropy(rows, y.repeat_interleave(loc), reduction="none").view(4, loc).mean(1)     # micro-batch 1: the mean over the image's windows
        loss64 = loss64 + per_image.sum() / 4 / 2                                                               # share 1/4 of the mini-batch, two scales averaged
    loss64.backward()
    print("scales step: loss %.8f, float64 %.8f" % (loss, float(loss64.detach())))
    assert abs(loss - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach()))
    ref = dict(("features.%d.%s" % (split + int(n.split(".", 1)[0]), n.split(".", 1)[1]), p.grad) for n, p in blocks64.named_parameters())
    ref.update(("classifier.0." + n, p.grad) for n, p in conv64.named_parameters())
    assert set(ref) == set(grads)
    worst = {}
    for n in sorted(grads):
        e = _rel(grads[n].double(), ref[n])
        kind = "classifier." + n.rsplit(".", 1)[1] if n.startswith("classifier") else ("conv" if grads[n].dim() > 1 else "bn")
        worst[kind] = max(worst.get(kind, 0.0), e)
    print("scales step vs float64 autograd, worst relative deviation per kind:", worst)
    for n in sorted(grads):
        assert _rel(grads[n].double(), ref[n]) <= _bound(n, grads[n]), (n, _rel(grads[n].double(), ref[n]))
    for n in grads:
        assert not torch.equal(after_on[n], start[n]), n                                    # the step moved every trainable tensor
    # the same step one micro-batch at a time (what a rank holding ONE leaf runs): the same bits
    net.load_state_dict(start)
    loss_leaf, grads_leaf = _step(net, xs, y, batched="leaf")
    assert loss_leaf == loss
    for n in grads:
        assert torch.equal(grads[n], grads_leaf[n]), n
    # engines on vs ISX_CLASSIF_ENGINE=0 (the generic route: pool, classifier and loss per micro-batch on torch autograd): same bounds
    net.load_state_dict(start)
    monkeypatch.setattr(siamese, "CLASSIF_ENGINE", False)
    assert net.classif_head_engine() is None
    loss_off, grads_off = _step(net, xs, y)
    print("region classifier engine on / off: loss %.8f / %.8f" % (loss, loss_off))
    assert abs(loss - loss_off) <= 1e-5 * abs(loss_off)
    assert set(grads_off) == set(grads)
    worst = max(_rel(grads[n], grads_off[n]) for n in grads)
    print("region classifier engine on vs off: worst relative gradient deviation %.3g" % worst)
    for n in grads:
        assert _rel(grads[n], grads_off[n]) <= _bound(n, grads[n]), (n, _rel(grads[n], grads_off[n]))


def test_entry_point_end_to_end(capsys, tmp_path):
    """train.classif_regions.run on a structured synthetic set, ResNet-50, one epoch of two steps: completes, logs, and its checkpoint is what
    train.siamese_regions loads as P.classif_model."""
    from train import _common as TC
    from train import classif_regions as cr
    from train import siamese_regions as sr
    saved, saved_labels = copy.copy(cr.P.__dict__), list(cr.labels)
    try:
        P = cr.P
        P.cuda_device, P.cnn_model, P.train_epochs, P.train_batch_size, P.train_micro_batch = 0, "resnet50", 1, 8, 1
        P.train_seed, P.train_annealing, P.train_loss_int, P.save_dir, P.train_sub_scales = 1, {}, 1, str(tmp_path), [None, 224]
        TC.drop_resident()
        torch.manual_seed(0)
        capsys.readouterr()
        net, _ = cr.run("synthetic:CLICIDE_video_224sq:n=16:q=4:labels=2:size=288:struct=60")
        out = capsys.readouterr().out
        assert net.classif_head_engine() is not None                                      # the run was on the engines' route
    finally:
        cr.P.__dict__.clear(); cr.P.__dict__.update(saved); cr.labels[:] = saved_labels
        TC.drop_resident()
    assert len(re.findall(r"^\[1, +\d+\] loss: \S+$", out, re.M)) == 2, out
    assert len(re.findall(r"^TEST - correct: \d+ / 4 - acc: ", out, re.M)) == 2 and len(re.findall(r"^TRAIN - correct: \d+ / 16 - acc: ", out, re.M)) == 2
    assert "Starting classification training" in out and "Finished classification training" in out and "Testing as descriptor" in out
    ckpt = os.path.join(str(tmp_path), "model_classif_1.pth.tar")
    state = torch.load(ckpt)
    saved = copy.copy(sr.P.__dict__)
    try:
        P = sr.P
        P.cuda_device, P.cnn_model, P.num_classes, P.classif_model, P.feature_dim, P.feature_size2d, P.preload_net = 0, "resnet50", 2, ckpt, 64, (7, 7), ""
        siam = sr.get_siamese_net()                                                         # load_state_dict is strict: a key error raises here
        mine = {k: v for k, v in siam.state_dict().items() if k.startswith(("features.", "classifier."))}
        assert mine and all(torch.equal(v.cpu(), state[k].cpu()) for k, v in mine.items())
    finally:
        sr.P.__dict__.clear(); sr.P.__dict__.update(saved)
