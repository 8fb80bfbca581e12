"""Classification fine-tuning on the GPU (csrc/classif.hip, isx/classif_head.py, TuneClassif's training hooks): the cross-entropy kernels against
F.cross_entropy in float64, leaf independence bit for bit, the per-leaf weight gradient against the oracle's canonical chain, one optimizer
step of TuneClassif(ResNet-50) on the engines against float64 autograd and against the torch-autograd tail, and the entry point end to end."""
import copy
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _logits(B, C, seed):
    """Rows of N(0, 3) scores; row 0 spread over +-80 (exp underflows for most classes), row 1 holds its label at the maximum, row 2 at the
    minimum of a +-80 spread."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    z[0] = torch.linspace(-80, 80, C)[torch.randperm(C, generator=g)]
    z[1, y[1]] = z[1].max() + 2.5
    z[2] = torch.linspace(-80, 80, C)[torch.randperm(C, generator=g)]
    y[2] = int(z[2].argmin())
    return z, y


@pytest.mark.parametrize("C", [17, 311, 464, 1000])
def test_cross_entropy_kernels_match_float64(C):
    """Arbiter: F.cross_entropy in float64.  e_cpu = the error of torch's own fp32 CPU F.cross_entropy against it; the kernels' error must be
    <= max(2 e_cpu, 4 fp32 ulps of the value) -- for the per-row losses, the per-leaf losses and the gradient."""
    from isx import ops
    leaves, k = 4, 8
    z, y = _logits(leaves * k, C, C)
    scale_a, scale_b = 1.0 / k, 0.25
    z64 = z.double().requires_grad_(True)
    rows64 = F.cross_entropy(z64, y, reduction="none")
    (rows64.sum() * (scale_a * scale_b)).backward()
    zc = z.clone().requires_grad_(True)
    rows_cpu = F.cross_entropy(zc, y, reduction="none")
    (rows_cpu.sum() * (scale_a * scale_b)).backward()
    zg, yg = z.cuda(), y.cuda()
    rows = ops.softmax_xent_rows(zg, yg).cpu()
    grad = ops.softmax_xent_grad(zg, yg, scale_a, scale_dev=torch.tensor([scale_b], device="cuda")).cpu()
    per_leaf, grad_l = ops.softmax_xent_leaves(zg, yg, leaves, scale_a, scale_b)
    assert torch.isfinite(rows).all() and torch.isfinite(grad).all() and torch.isfinite(per_leaf).all()
    assert torch.equal(grad_l.cpu(), grad)                                     # one arithmetic for a row, whichever entry computes it
    for what, got, cpu, ref in (("row losses", rows, rows_cpu.detach(), rows64.detach()),
                                ("leaf losses", per_leaf.cpu(), rows_cpu.detach().view(leaves, k).sum(1), rows64.detach().view(leaves, k).sum(1)),
                                ("gradient", grad, zc.grad, z64.grad)):
        e_gpu = float((got.double() - ref).abs().max())
        e_cpu = float((cpu.double() - ref).abs().max())
        print("cross-entropy C=%d %s: max |kernel - f64| = %.3g, max |torch CPU fp32 - f64| = %.3g" % (C, what, e_gpu, e_cpu))
        # per element: twice the CPU path's largest error, or -- the floor for e_cpu == 0 -- 4 fp32 ulps of that element's value
        floor = torch.from_numpy(4 * np.spacing(ref.abs().numpy().astype(np.float32)).astype(np.float64))
        over = (got.double() - ref).abs() > torch.clamp(floor, min=2 * e_cpu)
        assert not bool(over.any()), (what, e_gpu, e_cpu)
    # the module: libisx on fp32 GPU scores, forward value and gradient
    from model.custom_modules import CrossEntropyLoss
    for avg in (True, False):
        zm = zg.clone().requires_grad_(True)
        loss = CrossEntropyLoss(avg)(zm, yg)
        (loss * 0.25).backward()
        want = F.cross_entropy(z64.detach(), y, reduction="mean" if avg else "sum")
        assert abs(float(loss.detach()) - float(want)) <= 1e-5 * abs(float(want))
        assert torch.equal(zm.grad, ops.softmax_xent_grad(zg, yg, 1.0 / (leaves * k) if avg else 1.0, scale_dev=torch.tensor([0.25], device="cuda")))


def test_out_of_range_label_is_not_a_fault():
    from isx import ops
    z = torch.randn(4, 17, device="cuda")
    y = torch.tensor([0, 17, -1, 3], device="cuda")
    rows = ops.softmax_xent_rows(z, y)
    torch.cuda.synchronize()
    assert torch.isnan(rows[1]) and torch.isnan(rows[2]) and torch.isfinite(rows[0]) and torch.isfinite(rows[3])


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_leaves_launched_together_equal_leaves_launched_alone(L, k):
    """Bit-exact: cross-entropy, pool backward and the per-leaf weight gradient of leaf l do not depend on its siblings."""
    from isx import ops
    g = torch.Generator().manual_seed(100 * L + k)
    C, K = 464, 2048
    z = (torch.randn(L * k, C, generator=g) * 4).cuda()
    y = torch.randint(0, C, (L * k,), generator=g).cuda()
    per_leaf, dz = ops.softmax_xent_leaves(z, y, L, 1.0 / k, 1.0 / L)
    x = torch.randn(L * k, K, generator=g).cuda()
    dw = ops.linear_wgrad_leaves(dz, x, L)
    gp = torch.randn(L * k, K, generator=g).cuda()
    dx = ops.gap_bwd_nhwc(gp, 7, 7)
    assert dx.shape == (L * k, K, 7, 7) and dx.is_contiguous(memory_format=torch.channels_last)
    want = torch.from_numpy(gp.cpu().numpy() / np.float32(49.0))                            # IEEE fp32 division, one per element
    assert torch.equal(dx.cpu(), want.view(L * k, K, 1, 1).expand(L * k, K, 7, 7))
    for l in range(L):
        s = slice(l * k, (l + 1) * k)
        pl, dzl = ops.softmax_xent_leaves(z[s], y[s], 1, 1.0 / k, 1.0 / L)
        assert torch.equal(pl[0], per_leaf[l]) and torch.equal(dzl, dz[s])
        assert torch.equal(ops.linear_wgrad_leaves(dz[s], x[s], 1)[0], dw[l])
        assert torch.equal(ops.gap_bwd_nhwc(gp[s], 7, 7), dx[s])


@pytest.mark.parametrize("L,R,N,K", [(2, 13, 464, 2048), (3, 5, 311, 260), (1, 37, 17, 64)])
def test_linear_wgrad_leaves_is_the_oracles_chain(L, R, N, K):
    """dw[l] = oracle.cosine_sim(dy_l^T, x_l^T): a k-ordered fp32 fma chain from +0 with k = the leaf's row index -- bit for bit."""
    import oracle as O
    from isx import ops
    g = torch.Generator().manual_seed(R)
    dy, x = torch.randn(L * R, N, generator=g), torch.randn(L * R, K, generator=g)
    dw = ops.linear_wgrad_leaves(dy.cuda(), x.cuda(), L).cpu().numpy()
    for l in range(L):
        want = O.cosine_sim(np.ascontiguousarray(dy[l * R:(l + 1) * R].t().numpy()), np.ascontiguousarray(x[l * R:(l + 1) * R].t().numpy()))
        assert np.array_equal(dw[l], want), (l, float(np.abs(dw[l] - want).max()))


@pytest.mark.parametrize("N", [17, 64])
def test_one_engine_serves_linear_and_pointwise_conv(N, monkeypatch):
    """The same weights as nn.Linear behind AvgPool2d(7) and as 1x1 PointwiseConv behind BoxPool((7, 7), stride 1), 4 maps of 7 x 7 in 2 leaves:
    the same bits, the whole-map backward isx_gap_bwd_nhwc on the pooled gradient in both; a Linear on a map the pool does not span is an error.
    N = 17 takes the class-padding path, 64 the parameters as they are."""
    import types
    from isx import ops
    from isx._lib import IsxError
    from isx.classif_head import ClassifHeadEngine
    from model.siamese import BoxPool, PointwiseConv
    K, M, L = 64, 4, 2
    gen = torch.Generator().manual_seed(N)
    y_all = torch.randn(M, K, 7, 7, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, N, (M,), generator=gen).cuda()
    w, b = torch.randn(N, K, generator=gen) * (7.0 / K ** 0.5), torch.randn(N, generator=gen) * 0.1
    lin, conv = nn.Linear(K, N), PointwiseConv(K, N, 1)
    with torch.no_grad():
        lin.weight.copy_(w); lin.bias.copy_(b)
        conv.weight.copy_(w.view(N, K, 1, 1)); conv.bias.copy_(b)
    pooled_grads = []
    gap_bwd = ops.gap_bwd_nhwc
    monkeypatch.setattr(ops, "gap_bwd_nhwc", lambda g, H, W: (pooled_grads.append((g.clone(), H, W)), gap_bwd(g, H, W))[1])

    def run(pool, cls, y):
        holder = types.SimpleNamespace(feature_reduc=nn.Sequential(pool), classifier=nn.Sequential(cls).cuda())
        assert ClassifHeadEngine.applicable(holder)
        flat_all = torch.zeros(L, N * K + N, device="cuda")
        per_leaf, dy = ClassifHeadEngine(holder).step(y, labels, L, 0.5, 0.25, flat_all, {cls.weight: (0, N * K), cls.bias: (N * K, N * K + N)}, need_dy=True)
        return per_leaf, dy, flat_all

    pl_lin, dy_lin, flat_lin = run(nn.AvgPool2d(7), lin, y_all)
    pl_conv, dy_conv, flat_conv = run(BoxPool((7, 7), stride=1), conv, y_all)
    assert torch.equal(pl_lin, pl_conv) and torch.equal(dy_lin, dy_conv)
    assert bool(torch.isfinite(pl_lin).all()) and bool(flat_lin.abs().sum(1).gt(0).all())
    for l in range(L):
        assert torch.equal(flat_lin[l], flat_conv[l]), l
    assert len(pooled_grads) == 2                                                   # both tails took the whole-map backward
    for (g, H, W), dy in zip(pooled_grads, (dy_lin, dy_conv)):
        assert g.shape == (M, K) and (H, W) == (7, 7) and torch.equal(dy, gap_bwd(g, 7, 7))
    with pytest.raises(IsxError):
        run(nn.AvgPool2d(7), lin, torch.randn(M, K, 9, 9, generator=gen).cuda().contiguous(memory_format=torch.channels_last))


# ---- one optimizer step of TuneClassif(ResNet-50) --------------------------------------------------------------------------------------
def _calibrated(classes, x):
    """TuneClassif(ResNet-50) with seeded weights whose BatchNorm running statistics are those of the images x (one training-mode pass) and whose
    classifier is scaled to class scores of unit spread: the seeded default initialisation with identity statistics lets the activations grow
    by orders of magnitude per stage (first loss ~1e3, softmax saturated) -- gradients worth comparing need a net in its working range."""
    from isx import backbones
    from model.siamese import TuneClassif
    from train.params import UNTRAINED_BLOCKS
    torch.manual_seed(0)
    net = TuneClassif(backbones.resnet50(pretrained=True, seed=0), classes, untrained=UNTRAINED_BLOCKS["resnet50"]).cuda()
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
        scores = net(x)
        net.classifier[0].weight.div_(float(scores.std()) + 1e-12)
        net.classifier[0].bias.zero_()
    return net


def _net(classes, x):
    from model.nn_utils import set_net_train
    net = _calibrated(classes, x)
    set_net_train(net, True, bn_train=False)
    return net


def _step(net, x, y, batch=16, micro=8, batched=True):
    """One utils.train_general._Stepper step on images x / class indices y; returns (loss, {name: gradient}, the stepper).
    batched="leaf": the engines one micro-batch at a time (what a rank holding one leaf runs)."""
    from model.custom_modules import CrossEntropyLoss
    from train.params import Params
    from utils.train_general import _Stepper, make_sgd
    P = Params(cuda_device=0, train_batch_size=batch, train_micro_batch=micro, train_loss_avg=True, train_prefix_ahead=1, train_suffix_batched=batched)
    criterion = CrossEntropyLoss(True)

    def create_batch(items, n):
        idx = torch.tensor(items, device="cuda")
        return [x[idx]], [y[idx]]

    def create_loss(out, labels_list):
        return criterion(out, labels_list[0]), None
    create_loss.cross_entropy = criterion
    stepper = _Stepper(P, net, create_batch, create_loss)
    opt = make_sgd((p for p in net.parameters() if p.requires_grad), 1e-3, 0.0, 0.0)
    loss = stepper.step(opt, list(range(batch)), {})
    torch.cuda.synchronize()
    return float(loss), dict((n, p.grad.detach().clone()) for n, p in net.named_parameters() if p.requires_grad), stepper


def _bound(name, p):
    """The relative bounds tests/test_gpu_suffix.py asserts for the same kinds of tensor: 2e-5 for weight matrices (convolution / Linear),
    1e-5 for the small vectors (BatchNorm weight / bias, the classifier bias)."""
    return 2e-5 if p.dim() > 1 else 1e-5


def test_engine_step_matches_float64_autograd_and_the_autograd_tail(monkeypatch):
    from model import nn_utils
    from model import siamese
    from test_gpu_suffix import _ref64_with_masks, _rel
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(16, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 464, (16,), device="cuda", generator=g)
    net = _net(464, x)
    start = copy.deepcopy(net.state_dict())
    conv_calls = []
    hooks = [m.register_forward_hook(lambda m_, i_, o_: conv_calls.append(m_)) for m in net.features.modules() if isinstance(m, nn.Conv2d)]
    nn_utils.TORCH_CONV_CALLS.clear()
    loss, grads, stepper = _step(net, x, y)
    for h in hooks:
        h.remove()
    # no convolution of the ResNet-50 step ran on torch / MIOpen: TORCH_CONV_CALLS records the folded trunk's fall-backs (the frozen prefix), the
    # forward hooks the plain nn.Conv2d modules autograd would call (the recorder does not cover those)
    assert nn_utils.TORCH_CONV_CALLS == {} and conv_calls == []
    assert net.classif_head_engine() is not None and net.suffix_engine() is not None
    # float64 autograd on the same prefix features with the engine's ReLU pattern pinned
    net.load_state_dict(start)
    (f,) = net.precompute_trunk(x)
    split = net._trunk.split
    eng = net.suffix_engine()
    _, saved = eng.forward(f)
    masks = [tuple((t > 0).permute(0, 3, 1, 2).double() for t in (t1, t2, yb)) for _, t1, t2, yb in saved]
    blocks64 = copy.deepcopy(nn.Sequential(*list(net.features)[split:])).double()
    lin64 = copy.deepcopy(net.classifier[0]).double()
    y64 = _ref64_with_masks(blocks64, f.double(), masks)
    loss64 = F.cross_entropy(lin64(y64.mean((2, 3))), y)                          # mean over the 16 images = sum of the two leaves' shares
    loss64.backward()
    print("engine step: loss %.8f, float64 %.8f" % (loss, float(loss64.detach())))
    assert abs(loss - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach()))
    ref = dict(("features.%d.%s" % (split + int(n.split(".", 1)[0]), n.split(".", 1)[1]), p.grad) for n, p in blocks64.named_parameters())
    ref.update(("classifier.0." + n, p.grad) for n, p in lin64.named_parameters())
    assert set(ref) == set(grads)
    worst = {}
    for n in sorted(grads):
        e = _rel(grads[n].double(), ref[n])
        kind = "classifier." + n.rsplit(".", 1)[1] if n.startswith("classifier") else ("conv" if grads[n].dim() > 1 else "bn")
        worst[kind] = max(worst.get(kind, 0.0), e)
    print("engine step vs float64 autograd, worst relative deviation per kind:", worst)
    for n in sorted(grads):
        assert _rel(grads[n].double(), ref[n]) <= _bound(n, grads[n]), (n, _rel(grads[n].double(), ref[n]))
    # engines on vs ISX_CLASSIF_ENGINE=0 (pool, classifier and loss per micro-batch on torch autograd): same bounds
    net.load_state_dict(start)
    loss_on, grads_on, _ = _step(net, x, y)
    assert loss_on == loss and all(torch.equal(grads_on[n], grads[n]) for n in grads)      # the step is deterministic
    after_on = copy.deepcopy(net.state_dict())
    net.load_state_dict(start)
    monkeypatch.setattr(siamese, "CLASSIF_ENGINE", False)
    assert net.classif_head_engine() is None
    loss_off, grads_off, _ = _step(net, x, y)
    print("classifier engine on / off: loss %.8f / %.8f" % (loss_on, loss_off))
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    worst = max(_rel(grads_on[n], grads_off[n]) for n in grads)
    print("classifier engine on vs off: worst relative gradient deviation %.3g" % worst)
    for n in grads:
        assert _rel(grads_on[n], grads_off[n]) <= _bound(n, grads[n]), (n, _rel(grads_on[n], grads_off[n]))
    after_off = net.state_dict()
    for n in grads:
        assert _rel(after_on[n], after_off[n]) <= _bound(n, grads[n]), n
        assert not torch.equal(after_on[n], start[n]), n                                # the step moved every trainable tensor


def test_engine_step_leaf_by_leaf_is_bit_identical():
    """The step with all micro-batches in one pass == the same machinery one micro-batch at a time (what a rank holding ONE leaf runs)."""
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(16, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 311, (16,), device="cuda", generator=g)
    net = _net(311, x)
    start = copy.deepcopy(net.state_dict())
    loss, grads, _ = _step(net, x, y, micro=4)
    net.load_state_dict(start)
    loss1, grads1, _ = _step(net, x, y, micro=4, batched="leaf")
    assert loss1 == loss
    for n in grads:
        assert torch.equal(grads[n], grads1[n]), n


# the end-to-end run: structured synthetic images (per-label pattern share in per cent), epochs, mini-batch, learning rate
_E2E = {"struct": 60, "epochs": 3, "batch": 16, "lr": 1e-2, "n": 64, "labels": 4}


def _final_train_acc(out):
    got = re.findall(r"^TRAIN - correct: (\d+) / (\d+) - acc: ", out, re.M)
    return [int(c) for c, _ in got], int(got[0][1])


def test_fine_tuning_end_to_end_against_the_autograd_route(monkeypatch, capsys, tmp_path):
    """train.classif_finetune.main on a structured synthetic set, ResNet-50: the training accuracy rises above its upfront value, and the final
    TRAIN accuracy of the engine run lies within the band two autograd runs with different seeds span (at least one image) of the same-seed
    autograd run."""
    from model import siamese
    from train import _common as TC
    from train import classif_finetune as cf
    saved = copy.copy(cf.P.__dict__)
    spec = "synthetic:CLICIDE_video_224sq:n=%d:q=16:labels=%d:size=224:struct=%d" % (_E2E["n"], _E2E["labels"], _E2E["struct"])
    # the "ImageNet" weights of the run: seeded ResNet-50 with BatchNorm statistics of the training images (see _calibrated), from a file
    from utils.dataset import synthetic_image_set
    imgs = torch.stack([im for im, _, _ in synthetic_image_set(_E2E["n"], _E2E["labels"], (3, 224, 224), seed=1234, structure=_E2E["struct"] / 100.0)]).cuda()
    weights = str(tmp_path / "pretrained.pth.tar")
    torch.save(_calibrated(_E2E["labels"], imgs).state_dict(), weights)
    del imgs

    def run(seed, engines):
        monkeypatch.setattr(siamese, "CLASSIF_ENGINE", engines)
        monkeypatch.setattr(siamese, "SUFFIX_ENGINE", engines)
        cf.P.__dict__.clear(); cf.P.__dict__.update(copy.copy(saved))
        P = cf.P
        P.cuda_device, P.cnn_model, P.train_epochs, P.train_batch_size, P.train_micro_batch = 0, "resnet50", _E2E["epochs"], _E2E["batch"], 8
        P.train_lr, P.train_seed, P.train_annealing, P.test_descriptor_net, P.train_loss_int = _E2E["lr"], seed, {}, False, 1
        P.preload_net = weights
        TC.drop_resident()
        torch.manual_seed(0)
        capsys.readouterr()
        cf.run(spec)
        out = capsys.readouterr().out
        accs, total = _final_train_acc(out)
        _E2E.setdefault("losses", []).append(re.findall(r"loss: ([0-9.a-z]+)", out))
        return accs, total

    try:
        eng, total = run(1, True)
        ref1, _ = run(1, False)
        ref2, _ = run(2, False)
    finally:
        cf.P.__dict__.clear(); cf.P.__dict__.update(saved)
        TC.drop_resident()
    band = max(abs(ref1[-1] - ref2[-1]), 1)
    with capsys.disabled():
        print("fine-tuning ResNet-50, TRAIN correct of %d per evaluation: engines %s | autograd seed 1 %s | autograd seed 2 %s | band %d"
              % (total, eng, ref1, ref2, band))
    assert eng[-1] > eng[0], "training accuracy did not rise above its upfront value"
    assert abs(eng[-1] - ref1[-1]) <= band
