"""Region-descriptor siamese training on the GPU: isx_region_sum_l2_nhwc / isx_region_sum_l2_bwd_nhwc against their CPU model
(tests/_region_train_model.py) bit for bit and against float64 autograd; isx/region_head.RegionHeadEngine against float64 autograd of the
module's own torch path; one optimizer step of RegionDescriptorNet(TuneClassifSub(ResNet-50)) on the engine route against float64 autograd,
leaf by leaf, and against the generic route; two ranks against one process; train.siamese_regions.main end to end."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _guards as G
import _region_train_model as M

pytestmark = pytest.mark.gpu

EPS = 1e-10


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------------------
def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _launch(case, fmap, idx, Wp, shift, g, add, add_every=1):
    """Both entries through the C ABI on guarded buffers: (rows, n2, dfmap (B, C, Hf, Wf), cw) as host arrays."""
    from isx import _lib
    lib = _lib.lib()
    B, Hf, Wf, C, kh, kw, k = case
    Fd = C * kh * kw
    r_f, r_i, r_g = G.in_f32(_nhwc(fmap)), G.in_i64(idx), G.in_f32(g)
    r_s = G.in_f32(shift) if shift is not None else None
    r_a = G.in_f32(_nhwc(add)) if add is not None else None
    rows, n2 = G.out_f32((B, Fd), 4096), G.out_f32((B, k), 4096)
    rc = lib.isx_region_sum_l2_nhwc(r_f.ptr, B, C, Hf, Wf, kh, kw, r_i.ptr, k, Wp, G.ptr(r_s), EPS, rows.ptr, n2.ptr, None)
    assert rc == 0, lib.isx_last_error()
    G.assert_clean((rows, n2), (r_f, r_i, r_s), ("forward", case))
    r_n = G.in_f32(n2.host())
    cw, dfmap = G.out_f32((B, k), 4096), G.out_f32((B, Hf, Wf, C), 4096)
    rc = lib.isx_region_sum_l2_bwd_nhwc(r_f.ptr, r_g.ptr, r_n.ptr, B, C, Hf, Wf, kh, kw, r_i.ptr, k, Wp, G.ptr(r_a), add_every, cw.ptr, dfmap.ptr, None)
    assert rc == 0, lib.isx_last_error()
    G.assert_clean((cw, dfmap), (r_f, r_g, r_n, r_i, r_a), ("backward", case))
    return rows.host(), n2.host(), np.transpose(dfmap.host(), (0, 3, 1, 2)), cw.host()


def _autograd(fmap, idx, Wp, kh, kw, shift, g, add, dtype):
    """gather -> NormalizeL2 -> Shift -> sum over the windows on torch CPU autograd (the module's own formula), plus <map, add>: (rows, dfmap)."""
    x = torch.from_numpy(np.array(fmap)).to(dtype).requires_grad_(True)
    eps = float(np.float32(EPS))
    rows = []
    for b in range(x.size(0)):
        acc = None
        for fi in np.asarray(idx[b]).tolist():
            if fi < 0:
                continue
            r, c = fi // Wp, fi % Wp
            v = x[b, :, r:r + kh, c:c + kw].reshape(-1)
            t = v / torch.sqrt((v * v).sum() + eps)
            if shift is not None:
                t = t + torch.from_numpy(np.array(shift)).to(dtype)
            acc = t if acc is None else acc + t
        rows.append(acc)
    rows = torch.stack(rows)
    obj = (rows * torch.from_numpy(np.array(g)).to(dtype)).sum()
    if add is not None:
        obj = obj + (x * torch.from_numpy(np.array(add)).to(dtype)).sum()
    obj.backward()
    return rows.detach().numpy(), x.grad.numpy()


def _within(got, ref64, cpu32, what):
    """|got - f64| <= max(2 e_cpu, 4 ulp), e_cpu the largest error of torch's fp32 CPU result against the same float64."""
    e_gpu, e_cpu = np.abs(got.astype(np.float64) - ref64), float(np.abs(cpu32.astype(np.float64) - ref64).max())
    print("%s: max |kernel - f64| = %.3g, max |torch CPU fp32 - f64| = %.3g" % (what, float(e_gpu.max()), e_cpu))
    floor = 4 * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    assert not (e_gpu > np.maximum(floor, 2 * e_cpu)).any(), (what, float(e_gpu.max()), e_cpu)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernels_are_the_model_bit_for_bit(case):
    B, Hf, Wf, C, kh, kw, k = case
    fmap, idx, Wp, shift, g, add = M.make_case(case)
    if case == M.SKIP_CASE:
        assert (idx == -1).sum() == 1
    for with_opt in (True, False):                                           # with and without shift / add
        sh, ad = (shift, add) if with_opt else (None, None)
        rows, n2, dfmap, cw = _launch(case, fmap, idx, Wp, sh, g, ad)
        want_rows, want_n2 = M.region_sum_l2(fmap, kh, kw, idx, Wp, sh)
        want_df, want_cw = M.region_sum_l2_bwd(fmap, g, want_n2, kh, kw, idx, Wp, ad)
        G.assert_bits(n2, want_n2, ("n2", case, with_opt))
        G.assert_bits(rows, want_rows, ("rows", case, with_opt))
        G.assert_bits(cw, want_cw, ("cw", case, with_opt))
        G.assert_bits(dfmap, want_df, ("dfmap", case, with_opt))
        if B > 1:                                                            # each image alone: the bits it has in the batch
            for b in range(B):
                one = (1,) + tuple(case[1:])
                r1, n1, d1, c1 = _launch(one, fmap[b:b + 1], idx[b:b + 1], Wp, sh, g[b:b + 1], None if ad is None else ad[b:b + 1])
                G.assert_bits(r1, rows[b:b + 1], ("rows alone", case, b))
                G.assert_bits(n1, n2[b:b + 1], ("n2 alone", case, b))
                G.assert_bits(d1, dfmap[b:b + 1], ("dfmap alone", case, b))
                G.assert_bits(c1, cw[b:b + 1], ("cw alone", case, b))
        if with_opt and B % 3 == 0:                                          # one map per three images (the region head's anchors): the others add nothing
            _, _, d3, _ = _launch(case, fmap, idx, Wp, sh, g, ad[:B // 3], add_every=3)
            want3, _ = M.region_sum_l2_bwd(fmap, g, want_n2, kh, kw, idx, Wp, ad[:B // 3], add_every=3)
            G.assert_bits(d3, want3, ("dfmap, add_every 3", case))
            assert np.array_equal(G.bits(d3[0]), G.bits(M.region_sum_l2_bwd(fmap[:1], g[:1], want_n2[:1], kh, kw, idx[:1], Wp, ad[:1])[0][0]))
            assert np.array_equal(G.bits(d3[1:]), G.bits(M.region_sum_l2_bwd(fmap[1:], g[1:], want_n2[1:], kh, kw, idx[1:], Wp, None)[0]))
        # the float64 arbiter, every case
        r64, d64 = _autograd(fmap, idx, Wp, kh, kw, sh, g, ad, torch.float64)
        r32, d32 = _autograd(fmap, idx, Wp, kh, kw, sh, g, ad, torch.float32)
        _within(rows, r64, r32, "region_sum_l2 %s opt=%d" % (case, with_opt))
        _within(dfmap, d64, d32, "region_sum_l2_bwd %s opt=%d" % (case, with_opt))


def test_ops_wrappers_give_the_abi_bits():
    from isx import ops
    case = M.CASES[0]
    B, Hf, Wf, C, kh, kw, k = case
    fmap, idx, Wp, shift, g, add = M.make_case(case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x = dev(_nhwc(fmap)).permute(0, 3, 1, 2)
    rows, n2 = ops.region_sum_l2_nhwc(x, kh, kw, dev(idx), Wp, dev(shift))
    dx = ops.region_sum_l2_bwd_nhwc(x, dev(g), n2, kh, kw, dev(idx), Wp, add=dev(_nhwc(add)).permute(0, 3, 1, 2))
    assert dx.shape == x.shape and dx.permute(0, 2, 3, 1).is_contiguous()
    want_rows, want_n2 = M.region_sum_l2(fmap, kh, kw, idx, Wp, shift)
    want_df, _ = M.region_sum_l2_bwd(fmap, g, want_n2, kh, kw, idx, Wp, add)
    G.assert_bits(rows, want_rows, "rows")
    G.assert_bits(n2, want_n2, "n2")
    G.assert_bits(dx.contiguous(), want_df, "dfmap")


# ---- RegionHeadEngine: everything behind the trunk ---------------------------------------------------------------------------------------------------
MARGIN = 1.0            # unit descriptors: a.n - a.p + 1 > 0 for nearly every triplet, so the triplet branch carries a gradient
ALPHA = 0.5


class _Sink(object):
    """What RegionHeadEngine needs of isx.dp.RowSink: it keeps the Linear's (x, dy) rows."""
    def __init__(self, weight):
        self.weight, self.x, self.dy, self.leaf_ids = weight, [], [], []

    def accepts(self, w):
        return w is self.weight

    def shard_for(self, w):
        return None

    def add(self, w, x, dy):
        self.x.append(x.clone()); self.dy.append(dy.clone())


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _tail64(y64, flat_idx, Wo, k, conv64, shift64, w64, b64, labels, leaf, share, xent_mean, loss2_avg):
    """The module's own torch path (model/siamese.RegionDescriptorNet._single_image + train/siamese_regions.create_loss + _objective) in float64
    for the triplet `leaf` of y64 (rows 3 leaf .. 3 leaf + 2), the window indices GIVEN: (loss, triplet part, window part)."""
    from model.custom_modules import NormalizeL2
    l2 = NormalizeL2()
    descs, cls_anchor = [], None
    for m in range(3 * leaf, 3 * leaf + 3):
        x = y64[m:m + 1]
        c = F.conv2d(F.avg_pool2d(x, 7, 1), conv64[0], conv64[1])
        acc = 0
        for fi in flat_idx[m].tolist():
            r, col = fi // Wo, fi % Wo
            region = x[:, :, r:r + 7, col:col + 7].reshape(1, -1)
            acc = acc + F.linear(l2(region) + shift64, w64, b64)
        descs.append(l2(acc))
        if m == 3 * leaf:
            cls_anchor = c[0].reshape(c.size(1), -1)[:, flat_idx[m]].t()                     # (k, num_classes)
    a, p, n = descs
    trip = ((a * n).sum(1) - (a * p).sum(1) + MARGIN).clamp(min=0).sum()                    # one row: size_average divides by 1
    loss2 = F.cross_entropy(cls_anchor, labels[leaf:leaf + 1].expand(k), reduction="mean" if xent_mean else "sum")
    return trip * share + ALPHA * (loss2 * share if loss2_avg else loss2), trip, loss2


def test_engine_tail_matches_float64_and_leaves_are_independent():
    """RegionHeadEngine.step on a (4 leaves x 3, 2048, 9, 9) map, 17 classes, k = 6 of 9 windows, D = 64 against float64 autograd of the module's
    own torch path with the engine's window indices imposed: leaf losses 1e-5; classifier weight, d y_all and the sink's dY^T X 2e-5 of the
    tensor's largest entry; biases and Shift 1e-5; every leaf alone gives the bits it has among its siblings."""
    import types
    from isx.region_head import RegionHeadEngine
    from model.custom_modules import NormalizeL2, TripletLoss
    from model.siamese import BoxPool, PointwiseConv, _descriptor_head
    L, K, N, k, D = 4, 2048, 17, 6, 64
    M_ = 3 * L
    gen = torch.Generator().manual_seed(11)
    y_all = torch.relu(torch.randn(M_, K, 9, 9, generator=gen)).cuda().contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, N, (L,), generator=gen).cuda()
    conv = PointwiseConv(K, N, 1)
    head = _descriptor_head(K * 49, D)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(N, K, 1, 1, generator=gen) * (7.0 / K ** 0.5))       # class scores of unit spread
        conv.bias.copy_(torch.randn(N, generator=gen) * 0.1)
        head[1].param.copy_(torch.randn(K * 49, generator=gen) * 1e-3)
        # a head of unit-spread outputs, as a trained one: with a weight of nn.Linear's initial scale W s is ~0.01 next to k b, all descriptors
        # are b / |b| (a.p ~ a.n ~ 0.98) and the triplet gradient n - p is a difference of near-equal vectors -- torch's own fp32 CPU autograd is then
        # 2.7e-5 off float64 on the bias and Shift gradients; at this scale it is 3e-6 off (a.p, a.n ~ 0.8)
        head[2].weight.copy_(torch.randn(D, K * 49, generator=gen))
        head[2].bias.copy_(torch.randn(D, generator=gen) * 0.1)
    net = types.SimpleNamespace(k=k, feature_reduc=nn.Sequential(BoxPool((7, 7), stride=1)), classifier=nn.Sequential(conv).cuda(),
                                feature_reduc1=head.cuda(), feature_reduc2=NormalizeL2())
    assert RegionHeadEngine.applicable(net)
    eng = RegionHeadEngine(net)
    assert eng.fits(9, 9) and eng.fits(8, 9) and not eng.fits(8, 8) and not eng.fits(6, 20)
    shift, lin = head[1].param, head[2]
    params = [conv.weight, conv.bias, shift, lin.bias]
    slices, at = {}, 0
    for p in params:
        slices[p] = (at, at + p.numel()); at += p.numel()
    share = 0.25
    trip = TripletLoss(MARGIN, True)
    scales = ((1.0, share), (1.0 / k, ALPHA * share))

    def run(y, lab, leaves):
        flat_all = torch.zeros(leaves, at, device="cuda")
        sink = _Sink(lin.weight)
        per_t, per_x, dy, idx = eng.step(y, lab, leaves, trip, scales[0], scales[1], sink, flat_all, slices)
        return per_t, per_x, dy, idx, flat_all, sink

    per_t, per_x, dy, idx, flat_all, sink = run(y_all, labels, L)
    assert dy.shape == y_all.shape and dy.permute(0, 2, 3, 1).is_contiguous() and idx.shape == (M_, k)
    assert all(len(set(r)) == k and min(r) >= 0 and max(r) < 9 for r in idx.tolist())
    # float64 autograd of the module's own path, the engine's window indices imposed
    y64 = y_all.double().requires_grad_(True)
    leafs64 = [t.detach().double().requires_grad_(True) for t in (conv.weight, conv.bias, shift, lin.weight, lin.bias)]
    cw64, cb64, s64, w64, b64 = leafs64
    for l in range(L):
        loss, t64, x64 = _tail64(y64, idx, 3, k, (cw64, cb64), s64, w64, b64, labels, l, share, True, True)
        gy, gcw, gcb, gs, gw, gb = torch.autograd.grad(loss, [y64] + leafs64)
        got_loss = float(per_t[l]) * share + ALPHA * (float(per_x[l]) / k * share)
        assert float(t64.detach()) > 0
        loss = float(loss.detach())
        assert abs(got_loss - loss) <= 1e-5 * abs(loss), (l, got_loss, loss)
        x_l, dy_l = sink.x[0][3 * l:3 * l + 3].double(), sink.dy[0][3 * l:3 * l + 3].double()
        e = {"classifier weight": _rel(flat_all[l, slices[conv.weight][0]:slices[conv.weight][1]].double().view_as(gcw), gcw),
             "classifier bias": _rel(flat_all[l, slices[conv.bias][0]:slices[conv.bias][1]].double(), gcb),
             "shift": _rel(flat_all[l, slices[shift][0]:slices[shift][1]].double(), gs),
             "head bias": _rel(flat_all[l, slices[lin.bias][0]:slices[lin.bias][1]].double(), gb),
             "head dY^T X": _rel(dy_l.t() @ x_l, gw), "d y_all": _rel(dy[3 * l:3 * l + 3].double(), gy[3 * l:3 * l + 3])}
        print("region engine leaf %d: loss %.8f (f64 %.8f), relative deviations %s" % (l, got_loss, loss, {n_: "%.3g" % v for n_, v in e.items()}))
        assert e["classifier weight"] <= 2e-5 and e["head dY^T X"] <= 2e-5 and e["d y_all"] <= 2e-5
        assert e["classifier bias"] <= 1e-5 and e["shift"] <= 1e-5 and e["head bias"] <= 1e-5
        # the leaf launched alone: the same bits
        t1, x1, dy1, idx1, flat1, sink1 = run(y_all[3 * l:3 * l + 3], labels[l:l + 1], 1)
        assert torch.equal(idx1, idx[3 * l:3 * l + 3]) and torch.equal(t1[0], per_t[l]) and torch.equal(x1[0], per_x[l])
        assert torch.equal(dy1, dy[3 * l:3 * l + 3]) and torch.equal(flat1[0], flat_all[l])
        assert torch.equal(sink1.x[0], sink.x[0][3 * l:3 * l + 3]) and torch.equal(sink1.dy[0], sink.dy[0][3 * l:3 * l + 3])


# ---- one optimizer step of RegionDescriptorNet(TuneClassifSub(ResNet-50)) --------------------------------------------------------------------------------
_CLASSES = 17
_K, _D = 6, 64


def _region_net(classes, x):
    from model.siamese import RegionDescriptorNet
    from model.nn_utils import set_net_train
    from test_gpu_classif_regions import _calibrated
    from train.params import UNTRAINED_BLOCKS
    class_net = _calibrated(classes, x)
    torch.manual_seed(1)
    net = RegionDescriptorNet(class_net, _K, _D, (7, 7), untrained=UNTRAINED_BLOCKS["resnet50"]).cuda()
    with torch.no_grad():
        # the head in its working range, as _calibrated puts the classifier: unit-spread outputs.  At nn.Linear's initial scale W s is ~0.01
        # next to k b, every descriptor is b / |b| and the triplet gradient a difference of near-equal vectors (see the engine-tail test: torch's
        # own fp32 autograd is then 2.7e-5 off float64 on the bias and Shift gradients)
        net.feature_reduc1[2].weight.normal_(0.0, 1.0)
        net.feature_reduc1[2].bias.normal_(0.0, 0.1)
    set_net_train(net, True, bn_train=False)
    return net


def _make_loss(crit, crit2):
    def create_loss(out, labels_list):                                     # train/siamese_regions.py's
        loss = crit(*(d for d, _ in out))
        cls_all = out[0][1].squeeze(0).t()
        return loss, crit2(cls_all, labels_list[0].expand(cls_all.size(0)))
    create_loss.region_triplet = (crit, crit2)
    return create_loss


def _stepper(net, xs, y, n, batched=True, lr=1e-3, fused=False):
    from model.custom_modules import TripletLoss
    from train.params import Params
    from utils.train_general import _Stepper, make_sgd
    P = Params(cuda_device=0, train_batch_size=n, train_micro_batch=1, train_loss_avg=True, train_loss2_avg=True, train_loss2_alpha=ALPHA,
               train_prefix_ahead=1, train_suffix_batched=batched, train_fused_head_sgd=fused)

    def create_batch(items, n_):
        idx = torch.tensor(items, device="cuda")
        return [x[idx] for x in xs], [y[idx]]

    stepper = _Stepper(P, net, create_batch, _make_loss(TripletLoss(MARGIN, True), nn.CrossEntropyLoss(reduction="mean")))
    return stepper, make_sgd((p for p in net.parameters() if p.requires_grad), lr, 0.0, 0.0)


def _step(net, xs, y, batched=True, routes=None):
    """One _Stepper step on len(y) triplets, micro-batch 1; returns (loss, {name: gradient})."""
    from utils.train_general import _Stepper
    stepper, opt = _stepper(net, xs, y, y.numel(), batched)
    if routes is not None:
        real = stepper._route
        stepper._route = lambda *a: routes.append(real(*a)) or routes[-1]
    loss = stepper.step(opt, list(range(y.numel())), {})
    torch.cuda.synchronize()
    return float(loss), dict((n, p.grad.detach().clone()) for n, p in net.named_parameters() if p.requires_grad)


def _ref64_step(net, split, x_prefix, masks, idx, y):
    """float64 autograd of one step on 2 triplets from the prefix output x_prefix (6 images, leaf-major) with the ReLU pattern `masks` and the
    window indices `idx` pinned: (loss, {parameter name: gradient})."""
    from test_gpu_suffix import _ref64_with_masks
    blocks64 = copy.deepcopy(nn.Sequential(*list(net.features)[split:])).double()
    conv64 = copy.deepcopy(net.classifier[0]).double()
    s64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (net.feature_reduc1[1].param, net.feature_reduc1[2].weight, net.feature_reduc1[2].bias))
    y64 = _ref64_with_masks(blocks64, x_prefix.double(), masks)
    loss64 = sum(_tail64(y64, idx, 3, _K, (conv64.weight, conv64.bias), s64, w64, b64, y, l, 0.5, True, True)[0] for l in range(2))
    loss64.backward()
    ref = dict(("features.%d.%s" % (split + int(n.split(".", 1)[0]), n.split(".", 1)[1]), p.grad) for n, p in blocks64.named_parameters())
    ref.update(("classifier.0." + n, p.grad) for n, p in conv64.named_parameters())
    ref.update({"feature_reduc1.1.param": s64.grad, "feature_reduc1.2.weight": w64.grad, "feature_reduc1.2.bias": b64.grad})
    return float(loss64.detach()), ref


@pytest.fixture(scope="module")
def setup():
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = tuple(torch.randn(2, 3, 288, 288, device="cuda", generator=g) for _ in range(3))
    y = torch.randint(0, _CLASSES, (2,), device="cuda", generator=g)
    net = _region_net(_CLASSES, torch.cat(xs, 0)[:4])
    return net, copy.deepcopy(net.state_dict()), xs, y


def test_step_matches_float64_autograd_leaf_mode_and_the_generic_route(setup, monkeypatch):
    """One _Stepper step on 2 triplets at 288 x 288 (9 x 9 map), k = 6, D = 64, on the engine route: no torch convolution, the route object is
    _regions_batched, loss and every gradient against float64 autograd with the engine's ReLU pattern and window indices pinned (loss 1e-5,
    matrices 2e-5, vectors 1e-5), "leaf" mode bit-identical, and ISX_REGION_ENGINE=0 against the same arbiter within the same bounds.
    Measured on one MI355X: engine route worst 4.9e-6 (head vectors), generic route 5.5e-6; the two routes against each other, unpinned, 12 %."""
    import functools
    from model import nn_utils, siamese
    from test_gpu_classif_regions import _bound
    from utils.train_general import _Stepper
    net, start, xs, y = setup
    net.load_state_dict(start)
    conv_calls, routes = [], []
    hooks = [m.register_forward_hook(lambda m_, i_, o_: conv_calls.append(m_)) for m in net.modules() if isinstance(m, nn.Conv2d)]
    nn_utils.TORCH_CONV_CALLS.clear()
    loss, grads = _step(net, xs, y, routes=routes)
    for h in hooks:
        h.remove()
    assert nn_utils.TORCH_CONV_CALLS == {} and conv_calls == []              # no convolution of the step ran on torch / MIOpen
    assert len(routes) == 1 and isinstance(routes[0], functools.partial) and routes[0].func.__func__ is _Stepper._regions_batched
    rhead, eng = net.region_head_engine(), net.suffix_engine()
    assert rhead is not None and eng is not None
    # float64 autograd on the same prefix features, the engine's ReLU pattern and window indices pinned
    net.load_state_dict(start)
    feats = net.precompute_trunk(*xs)
    assert [tuple(f.shape[2:]) for f in feats] == [(18, 18)] * 3
    x_all = torch.cat([f[o:o + 1] for o in range(2) for f in feats], 0)      # leaf-major
    y_all, saved = eng.forward(x_all)
    assert tuple(y_all.shape[2:]) == (9, 9)
    _, logits, _ = rhead.chead.scores(y_all)
    from isx import ops
    idx, _ = ops.region_topk(logits.view(6, 3, 3, _CLASSES).permute(0, 3, 1, 2), _K)
    split = net._trunk.split
    masks = [tuple((t > 0).permute(0, 3, 1, 2).double() for t in (t1, t2, yb)) for _, t1, t2, yb in saved]
    loss64, ref = _ref64_step(net, split, x_all, masks, idx, y)
    print("region step: loss %.8f, float64 %.8f" % (loss, loss64))
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert set(grads) <= set(ref) and "feature_reduc1.2.weight" in grads and any(n.startswith("features.") for n in grads)
    worst = {}
    for n in sorted(grads):
        kind = n.split(".")[0] + (" matrix" if grads[n].dim() > 1 else " vector")
        worst[kind] = max(worst.get(kind, 0.0), _rel(grads[n].double(), ref[n]))
    print("region step vs float64 autograd, worst relative deviation per kind:", worst)
    for n in sorted(grads):
        assert _rel(grads[n].double(), ref[n]) <= _bound(n, grads[n]), (n, _rel(grads[n].double(), ref[n]))
    # the same step one leaf at a time (what a rank holding ONE leaf runs): the same bits
    net.load_state_dict(start)
    loss_leaf, grads_leaf = _step(net, xs, y, batched="leaf")
    assert loss_leaf == loss
    for n in grads:
        assert torch.equal(grads[n], grads_leaf[n]), n
    # ISX_REGION_ENGINE=0: the generic route (the whole net on torch autograd / MIOpen, image by image) against the same arbiter within the same
    # bounds: float64 autograd with ITS ReLU pattern and ITS window indices pinned, on ITS prefix output -- all three recorded by hooks while the
    # step runs.  (The two fp32 routes are not compared gradient against gradient: their trunks round differently -- the prefix outputs differ by
    # 3.5e-5 of their largest entry -- and ~130 of the 5.3 M ReLU units of layer4 fall on the other side of 0, which moves the convolution
    # gradients of these two triplets by up to 12 % (an unpinned fp32 comparison measures the flips).  The figure is printed.)
    net.load_state_dict(start)
    monkeypatch.setattr(siamese, "REGION_ENGINE", False)
    assert net.region_head_engine() is None
    cap = {"f": [], "relu": [], "c": []}
    blocks = list(net.features)[split:]
    hooks = [net.features[split - 1].register_forward_hook(lambda m_, i_, o_: cap["f"].append(o_.detach().clone())),
             net.classifier.register_forward_hook(lambda m_, i_, o_: cap["c"].append(o_.detach().clone()))]
    hooks += [b.relu.register_forward_hook(lambda m_, i_, o_: cap["relu"].append((o_.detach() > 0).double())) for b in blocks]
    routes = []
    loss_off, grads_off = _step(net, xs, y, routes=routes)
    for h in hooks:
        h.remove()
    nb = len(blocks)
    assert routes == [None] and len(cap["f"]) == 6 and len(cap["c"]) == 6 and len(cap["relu"]) == 6 * 3 * nb      # image by image, leaf-major
    masks_off = [tuple(torch.cat([cap["relu"][m * 3 * nb + 3 * i + j] for m in range(6)], 0) for j in range(3)) for i in range(nb)]
    idx_off = torch.stack([c[0].max(0)[0].view(-1).sort(descending=True, stable=True)[1][:_K] for c in cap["c"]])
    net.load_state_dict(start)                                              # the reference reads the weights the step started from
    loss64_off, ref_off = _ref64_step(net, split, torch.cat(cap["f"], 0), masks_off, idx_off, y)
    print("region engine on / off: loss %.8f / %.8f (float64 of the generic route's pattern %.8f)" % (loss, loss_off, loss64_off))
    assert torch.equal(idx_off, idx)                                        # both routes chose the same windows, in the same order
    assert abs(loss_off - loss64_off) <= 1e-5 * abs(loss64_off) and abs(loss - loss_off) <= 1e-5 * abs(loss_off)
    assert set(grads_off) == set(grads)
    print("region engine on vs off, unpinned: worst relative gradient deviation %.3g" % max(_rel(grads[n], grads_off[n]) for n in grads))
    print("generic route vs float64 autograd of its own pattern: worst relative deviation %.3g" % max(_rel(grads_off[n].double(), ref_off[n]) for n in grads))
    for n in sorted(grads_off):
        assert _rel(grads_off[n].double(), ref_off[n]) <= _bound(n, grads_off[n]), (n, _rel(grads_off[n].double(), ref_off[n]))


# ---- two ranks on the one GPU against one process ------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, path, D):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from isx import dp as _dp
        blob = torch.load(path)
        xs, y = tuple(x.cuda() for x in blob["xs"]), blob["y"].cuda()
        net = _region_skeleton(D)
        net.load_state_dict(blob["start"])
        stepper, opt = _stepper(net, xs, y, 4, lr=1e-2, fused=True)
        stepper.step(opt, [0, 1, 2, 3], {})
        stepper.sync_head()                                                 # a sharded head: every rank's rows of the weight to every rank
        torch.cuda.synchronize()
        assert net.region_head_engine() is not None
        if rank == 0:
            torch.save({k: v.cpu() for k, v in net.state_dict().items()}, path + ".out")
            torch.save(dict(_dp.STATS), path + ".stats")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _region_skeleton(D=_D):
    from isx import backbones
    from model.nn_utils import set_net_train
    from model.siamese import RegionDescriptorNet, TuneClassifSub
    from train.params import UNTRAINED_BLOCKS
    u = UNTRAINED_BLOCKS["resnet50"]
    net = RegionDescriptorNet(TuneClassifSub(backbones.resnet50(pretrained=True, seed=0), _CLASSES, (7, 7), untrained=u), _K, D, (7, 7), untrained=u).cuda()
    set_net_train(net, True, bn_train=False)
    return net


@pytest.mark.parametrize("D", (_D, 256))
def test_two_ranks_on_one_gpu_match_single_process(setup, tmp_path, D):
    """4 triplets, one optimizer step: two ranks on the one GPU (gloo) against one process, the whole state dict bit for bit.  D = 256: a head
    wide enough for the 8 feature groups -- the ranks run it SHARDED by output features (isx/shard_head.py, through HeadEngine.linear_l2 with
    k = 6: the shard adds b once, the engine (k - 1) b), the single process the plain kernels."""
    import torch.multiprocessing as mp
    from test_training import _free_port
    net64, start64, xs2, y2 = setup
    if D == _D:
        net, start = net64, start64
    else:                                                                   # the calibrated trunk and classifier of the fixture under a wider head
        net = _region_skeleton(D)
        state = {k_: v for k_, v in start64.items() if not k_.startswith("feature_reduc1.")}
        net.load_state_dict(state, strict=False)
        with torch.no_grad():
            torch.manual_seed(2)
            net.feature_reduc1[2].weight.normal_(0.0, 1.0)
            net.feature_reduc1[2].bias.normal_(0.0, 0.1)
        start = copy.deepcopy(net.state_dict())
    g = torch.Generator(device="cuda").manual_seed(9)
    xs = tuple(torch.cat([x, torch.randn(2, 3, 288, 288, device="cuda", generator=g)], 0) for x in xs2)
    y = torch.cat([y2, torch.randint(0, _CLASSES, (2,), device="cuda", generator=g)], 0)
    path = str(tmp_path / "dp.pt")
    torch.save({"xs": [x.cpu() for x in xs], "y": y.cpu(), "start": {k: v.cpu() for k, v in start.items()}}, path)
    mp.spawn(_two_rank_worker, args=(2, _free_port(), path, D), nprocs=2, join=True)
    two = torch.load(path + ".out")
    assert (torch.load(path + ".stats").get("head_shard_bytes_received", 0) > 0) == (D % 256 == 0)
    net.load_state_dict(start)
    stepper, opt = _stepper(net, xs, y, 4, lr=1e-2, fused=True)
    stepper.step(opt, [0, 1, 2, 3], {})
    torch.cuda.synchronize()
    moved = 0.0
    for k_, v in net.state_dict().items():
        assert torch.equal(v.cpu(), two[k_]), (k_, float((v.cpu().float() - two[k_].float()).abs().max()))
        if v.dtype.is_floating_point:
            moved = max(moved, float((v - start[k_].to(v.device)).abs().max()))
    assert moved > 0


# ---- the main ---------------------------------------------------------------------------------------------------------------------------------------------
def test_main_runs_on_the_engine_route(monkeypatch):
    import random
    from train import _common as TC
    from train import siamese_regions as sr
    from utils.dataset import synthetic_image_set
    from utils.train_general import _Stepper
    saved, saved_labels = copy.copy(sr.P.__dict__), list(sr.labels)
    calls, real, nets = [], _Stepper._regions_batched, []
    monkeypatch.setattr(_Stepper, "_regions_batched", lambda self, *a: calls.append(len(a[-2])) or real(self, *a))
    real_net = sr.get_siamese_net

    def get_net():
        nets.append(real_net())
        nets.append(copy.deepcopy(nets[0].state_dict()))
        return nets[0]

    monkeypatch.setattr(sr, "get_siamese_net", get_net)
    try:
        torch.manual_seed(0); random.seed(0)
        P = sr.P
        P.cuda_device, P.cnn_model, P.feature_size2d, P.feature_dim, P.regions_k = 0, "resnet50", (7, 7), _D, _K
        P.train_epochs, P.train_batch_size, P.test_batch_size, P.train_loss_int, P.train_seed, P.train_annealing = 1, 4, 4, 1000, 1, {}
        P.untrained_blocks = None                                  # the reference's table
        P.train_lr, P.train_epoch_switch = 1e-7, 1                  # (random-init ResNet-50: see tests/test_training.py::test_region_training_runs_on_gpu)
        TC.drop_resident()
        tr = synthetic_image_set(8, 2, size=(3, 288, 288), seed=1, structure=0.6)
        te = synthetic_image_set(4, 2, size=(3, 288, 288), seed=2, structure=0.6)
        net, score = sr.main(tr, tr, te)
    finally:
        sr.P.__dict__.clear(); sr.P.__dict__.update(saved); sr.labels[:] = saved_labels
        TC.drop_resident()
    assert score >= 0 and calls and all(c == 4 for c in calls)                  # every step took the engine route, 4 leaves at a time
    assert net is nets[0] and net.region_head_engine() is not None
    after = net.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.dtype.is_floating_point)
    assert any(not torch.equal(after[k_], nets[1][k_]) for k_ in after)         # the weights moved
