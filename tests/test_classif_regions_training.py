"""Sub-region classifier training (pipeline stage 2) without a GPU: argument validation of isx_boxpool_s1_bwd_nhwc, the multi-scale loss against
F.cross_entropy in float64, the `python -m train.classif_regions` entry point end to end (log lines, checkpoints), the hand-over of its
checkpoint to the region-descriptor training (`P.classif_model` of train.siamese_regions) and the data-parallel (gloo) step against a single
process."""
import copy
import math
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instance-search_amd")


def _env():
    env = dict(os.environ, PYTHONPATH=PKG, OMP_NUM_THREADS="4", MKL_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_boxpool_backward_entry_validates_its_arguments_without_gpu():
    from isx import _lib, ops
    lib = _lib.lib()
    assert "isx_boxpool_s1_bwd_nhwc" in _lib.EXPORTS
    err = lib.isx_last_error
    assert lib.isx_boxpool_s1_bwd_nhwc(None, 2, 6, 14, 14, 7, 7, None, None) == -1 and b"multiple of 4" in err()
    assert lib.isx_boxpool_s1_bwd_nhwc(None, 2, 2048, 6, 14, 7, 7, None, None) == -1 and b"bad shape" in err()       # kh > H
    assert lib.isx_boxpool_s1_bwd_nhwc(None, 2, 2048, 14, 6, 7, 7, None, None) == -1 and b"bad shape" in err()       # kw > W
    assert lib.isx_boxpool_s1_bwd_nhwc(None, -1, 2048, 14, 14, 7, 7, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_boxpool_s1_bwd_nhwc(None, 2, 2048, 14, 14, 7, 7, None, None) == -1 and b"null" in err()
    buf = torch.zeros(64)                                                                   # a host buffer: rejected before any launch
    assert lib.isx_boxpool_s1_bwd_nhwc(buf.data_ptr(), 1, 4, 2, 2, 1, 1, buf.data_ptr(), None) == -1 and b"aliased" in err()
    assert lib.isx_boxpool_s1_bwd_nhwc(buf.data_ptr(), 1, 4, 2, 2, 1, 1, None, None) == -1 and b"null" in err()
    assert lib.isx_boxpool_s1_bwd_nhwc(None, 0, 2048, 14, 14, 7, 7, None, None) == 0         # B == 0: a no-op
    with pytest.raises(_lib.IsxError):
        ops.boxpool_s1_bwd_nhwc(torch.zeros(1, 8, 2, 2), 3, 3, 2, 2)                        # CPU tensors: no CPU path in libisx


@pytest.mark.parametrize("loss_avg", [True, False])
def test_region_loss_is_the_references_formula(loss_avg):
    """Score maps (1, 5, 3, 3) and (1, 5, 1, 1) in float64: (CE_mean(9 rows) + CE_mean(1 row)) / 2 with train_loss_avg, the plain sum of the
    reduction='sum' values without -- value and gradient."""
    from model.custom_modules import CrossEntropyLoss
    from train import classif_regions as cr
    g = torch.Generator().manual_seed(11)
    maps = [torch.randn(1, 5, 3, 3, generator=g, dtype=torch.float64) * 3, torch.randn(1, 5, 1, 1, generator=g, dtype=torch.float64) * 3]
    lab = torch.tensor([3])
    criterion = CrossEntropyLoss(size_average=loss_avg)
    create_loss = cr.region_loss(criterion, loss_avg)
    assert create_loss.region_cross_entropy is criterion
    assert not hasattr(cr.region_loss(nn.CrossEntropyLoss(), loss_avg), "region_cross_entropy")       # only THE criterion is declared
    got_in = [m.clone().requires_grad_(True) for m in maps]
    got, second = create_loss(got_in, [lab])
    assert second is None
    ref_in = [m.clone().requires_grad_(True) for m in maps]
    rows = [m[0].reshape(5, -1).t() for m in ref_in]
    red = "mean" if loss_avg else "sum"
    want = F.cross_entropy(rows[0], lab.expand(9), reduction=red) + F.cross_entropy(rows[1], lab.expand(1), reduction=red)
    if loss_avg:
        want = want / 2
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-14 * abs(float(want.detach()))
    got.backward()
    want.backward()
    for a, b in zip(got_in, ref_in):
        assert torch.allclose(a.grad, b.grad, rtol=1e-13, atol=1e-16)
    # several images per micro-batch: the mean over all windows of the micro-batch, every image's windows carrying its own label
    two = [torch.cat([m, m.flip(1)], 0) for m in maps]
    labs = torch.tensor([3, 1])
    got2, _ = create_loss(two, [labs])
    parts = [F.cross_entropy(t.flatten(2).permute(0, 2, 1).reshape(-1, 5), labs.repeat_interleave(t.size(2) * t.size(3)), reduction=red) for t in two]
    want2 = (parts[0] + parts[1]) / 2 if loss_avg else parts[0] + parts[1]
    assert abs(float(got2) - float(want2)) <= 1e-14 * abs(float(want2))


_SPEC = "synthetic:CLICIDE_video_224sq:n=8:q=4:labels=2:size=288:struct=100"


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One CPU run of the entry point: AlexNet at 288 -> an 8 x 8 map -> 3 x 3 windows; at 224 -> one window."""
    save = tmp_path_factory.mktemp("classif_regions")
    cmd = [sys.executable, "-m", "train.classif_regions", "--dataset=" + _SPEC, "--model=alexnet", "--device=-1", "--epochs=2", "--batch-size=4",
           "--scales=0,224", "--loss-int=1", "--seed=1", "--save-dir=" + str(save)]
    run = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout, save


def test_entry_point_trains_logs_and_checkpoints(trained):
    out, save = trained
    losses = [(int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in re.finditer(r"^\[(\d+), +(\d+)\] loss: (\S+)$", out, re.M)]
    assert [(e, s) for e, s, _ in losses] == [(1, 1), (1, 2), (2, 1), (2, 2)], out               # 8 images / batch 4 = two steps per epoch
    assert all(math.isfinite(l) for _, _, l in losses), losses
    tests = re.findall(r"^TEST - correct: (\d+) / (\d+) - acc: ([0-9.]+)$", out, re.M)
    trains = re.findall(r"^TRAIN - correct: (\d+) / (\d+) - acc: ([0-9.]+)$", out, re.M)
    assert len(tests) == 3 and len(trains) == 3                                                 # upfront + one evaluation per epoch
    assert all(t == "4" for _, t, _ in tests) and all(t == "8" for _, t, _ in trains)
    assert "Starting classification training" in out and "Finished classification training" in out and "Testing as descriptor" in out
    files = sorted(os.listdir(str(save)))
    assert len([f for f in files if f.endswith("_best_classif.pth.tar")]) == 1, files
    assert all("model_classif_%d.pth.tar" % e in files for e in range(3)), files


def test_checkpoint_feeds_the_next_stages(trained):
    """model_classif_2.pth.tar loads into get_class_net() (P.preload_net) and into the TuneClassifSub inside train.siamese_regions'
    get_siamese_net() (P.classif_model); its keys are those of a fresh TuneClassifSub."""
    _, save = trained
    ckpt = os.path.join(str(save), "model_classif_2.pth.tar")
    state = torch.load(ckpt)
    from isx import backbones
    from model.siamese import TuneClassifSub
    from train import classif_regions as cr
    from train import siamese_regions as sr
    fresh = TuneClassifSub(backbones.alexnet(pretrained=True), 2, (6, 6))
    assert list(state) == list(fresh.state_dict())
    saved, saved_labels = copy.copy(cr.P.__dict__), list(cr.labels)
    try:
        cr.P.cuda_device, cr.P.cnn_model, cr.P.feature_size2d, cr.P.bn_model, cr.P.preload_net = -1, "alexnet", (6, 6), "", ckpt
        cr.labels[:] = ["c000", "c001"]
        net = cr.get_class_net()
        assert all(torch.equal(v, state[k]) for k, v in net.state_dict().items())
    finally:
        cr.P.__dict__.clear(); cr.P.__dict__.update(saved); cr.labels[:] = saved_labels
    saved = copy.copy(sr.P.__dict__)
    try:
        P = sr.P
        P.cuda_device, P.cnn_model, P.num_classes, P.classif_model, P.feature_dim, P.feature_size2d, P.preload_net = -1, "alexnet", 2, ckpt, 16, (6, 6), ""
        net = sr.get_siamese_net()                                                  # load_state_dict is strict: a key error raises here
        mine = {k: v for k, v in net.state_dict().items() if k.startswith(("features.", "classifier."))}
        assert mine and all(torch.equal(v, state[k]) for k, v in mine.items())
    finally:
        sr.P.__dict__.clear(); sr.P.__dict__.update(saved)


class _TinyBackbone(nn.Module):
    """A backbone with the three parts extract_layers looks for: TuneClassifSub wraps it like a ResNet (pool + one Linear)."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv2d(3, 4, 3, stride=2), nn.BatchNorm2d(4), nn.ReLU())
        self.feature_reduc = nn.Sequential(nn.AvgPool2d(3))
        self.classifier = nn.Sequential(nn.Linear(4, 4))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run_regions(rank, world, port, out):
    sys.path.insert(0, PKG)
    torch.set_num_threads(1)
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch.optim as optim
    import utils.train_general as tg
    from model.custom_modules import CrossEntropyLoss
    from model.siamese import TuneClassifSub
    from train import classif_regions as cr
    torch.manual_seed(1000 * rank)                      # replicas start from DIFFERENT weights: train_gen broadcasts rank 0's
    net = TuneClassifSub(_TinyBackbone(), 4, (3, 3), untrained=0)
    P = cr.P
    P.cuda_device, P.train_epochs, P.train_batch_size, P.train_micro_batch, P.train_seed = -1, 1, 4, 1, 5
    P.train_loss_int, P.train_test_int, P.train_pre_proc, P.train_loss_avg, P.train_bn, P.train_annealing = 1000, 1000, True, True, False, {}
    g = torch.Generator().manual_seed(1)
    # 12 x 12 -> a 5 x 5 map -> 3 x 3 windows; its 8 x 8 scale -> a 3 x 3 map -> one window
    ds = [([torch.randn(3, 12, 12, generator=g), torch.randn(3, 8, 8, generator=g)], "l%d" % i, "p%d" % i) for i in range(4)]
    gallery = [(item[0][0], item[1], item[2]) for item in ds]
    cr.labels[:] = sorted(set(l for _, l, _ in ds))
    steps = []
    real_step = tg._Stepper.step
    tg._Stepper.step = lambda self, *a, **k: steps.append(1) or real_step(self, *a, **k)
    opt = optim.SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    if rank == 0:
        torch.save({k: v.clone() for k, v in net.state_dict().items()}, out + ".init")
    cr.train_classif_subparts(net, ds, (gallery[:2], gallery), CrossEntropyLoss(True), opt)
    assert len(steps) == 1
    torch.save({k: v.clone() for k, v in net.state_dict().items()}, out + ".%d" % rank)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_data_parallel_region_step_is_bit_identical_to_single_process(tmp_path):
    """gloo, world size 1 vs 2, 4 images, batch 4, micro-batch 1, train_seed fixed: every tensor after the optimizer step is the same bits (the
    leaves' gradients meet in the tree order of isx/dp.py whatever the number of ranks)."""
    single, dp = str(tmp_path / "single.pt"), str(tmp_path / "dp.pt")
    mp.spawn(_run_regions, args=(1, 0, single), nprocs=1, join=True)
    mp.spawn(_run_regions, args=(2, _free_port(), dp), nprocs=2, join=True)
    a = torch.load(single + ".0")
    init = torch.load(single + ".init")
    assert sum(float((a[k].float() - init[k].float()).abs().sum()) for k in a) > 1e-3          # training really changed the weights
    for r in range(2):
        b = torch.load(dp + ".%d" % r)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (r, k, float((a[k].float() - b[k].float()).abs().max()))
