"""Classification fine-tuning (pipeline stage 1) without a GPU: argument validation of the new libisx entries, the CrossEntropyLoss module on
CPU tensors, the `python -m train.classif_finetune` entry point end to end (log lines, checkpoints, decreasing loss), the hand-over of its
checkpoint to the siamese training (`--classif-model`) and the data-parallel (gloo) step against a single process."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instance-search_amd")


def _env():
    env = dict(os.environ, PYTHONPATH=PKG, OMP_NUM_THREADS="4", MKL_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_new_entries_validate_their_arguments_without_gpu():
    from isx import _lib
    lib = _lib.lib()
    for name in ("isx_softmax_xent_fwd", "isx_softmax_xent_bwd", "isx_softmax_xent_leaves", "isx_gap_bwd_nhwc", "isx_linear_wgrad_leaves"):
        assert name in _lib.EXPORTS
    err = lib.isx_last_error
    assert lib.isx_softmax_xent_fwd(None, None, -1, 4, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_softmax_xent_fwd(None, None, 4, 0, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_softmax_xent_fwd(None, None, 4, 17, None, None) == -1 and b"null pointer" in err()
    assert lib.isx_softmax_xent_fwd(None, None, 0, 17, None, None) == 0
    assert lib.isx_softmax_xent_bwd(None, None, 4, -3, 1.0, None, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_softmax_xent_bwd(None, None, 4, 17, 1.0, None, None, None) == -1 and b"null pointer" in err()
    assert lib.isx_softmax_xent_bwd(None, None, 0, 17, 1.0, None, None, None) == 0
    assert lib.isx_softmax_xent_leaves(None, None, 2, 0, 464, 1.0, 1.0, None, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_softmax_xent_leaves(None, None, 2, 9000, 464, 1.0, 1.0, None, None, None) == -1 and b"8192" in err()
    assert lib.isx_softmax_xent_leaves(None, None, -1, 8, 464, 1.0, 1.0, None, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_softmax_xent_leaves(None, None, 2, 8, 464, 1.0, 1.0, None, None, None) == -1 and b"null pointer" in err()
    assert lib.isx_softmax_xent_leaves(None, None, 0, 8, 464, 1.0, 1.0, None, None, None) == 0           # leaves == 0: a no-op
    # dlogits == logits is refused (the kernels take both as __restrict__; the leaves kernel reads z_label while other lanes write their dz)
    import ctypes
    buf = (ctypes.c_float * 64)()
    ptr, other = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(ctypes.addressof(buf) + 128)
    assert lib.isx_softmax_xent_bwd(ptr, other, 1, 4, 1.0, None, ptr, None) == -1 and b"aliases" in err()
    assert lib.isx_softmax_xent_leaves(ptr, other, 1, 1, 4, 1.0, 1.0, other, ptr, None) == -1 and b"aliases" in err()
    # the test hook for the device's expf / logf
    assert "isx_debug_expf_logf" in _lib.EXPORTS
    assert lib.isx_debug_expf_logf(ptr, -1, ptr, ptr, None) == -1 and b"bad shape" in err()
    assert lib.isx_debug_expf_logf(None, 4, ptr, ptr, None) == -1 and b"null pointer" in err()
    assert lib.isx_debug_expf_logf(None, 0, None, None, None) == 0
    assert lib.isx_gap_bwd_nhwc(None, 2, 7, 0, 2048, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_gap_bwd_nhwc(None, 2, 7, 7, 2046, None, None) == -1 and b"multiple of 4" in err()
    assert lib.isx_gap_bwd_nhwc(None, 2, 7, 7, 2048, None, None) == -1 and b"null" in err()
    assert lib.isx_gap_bwd_nhwc(None, 0, 7, 7, 2048, None, None) == 0
    assert lib.isx_linear_wgrad_leaves(None, None, 2, 0, 464, 2048, None, None) == -1 and b"bad shape" in err()
    assert lib.isx_linear_wgrad_leaves(None, None, 2, 8, 464, 2046, None, None) == -1 and b"multiple of 4" in err()
    assert lib.isx_linear_wgrad_leaves(None, None, 2, 8, 464, 2048, None, None) == -1 and b"null" in err()
    assert lib.isx_linear_wgrad_leaves(None, None, 0, 8, 464, 2048, None, None) == 0
    from isx import ops
    with pytest.raises(_lib.IsxError):
        ops.softmax_xent_rows(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64))                      # CPU tensors: no CPU path in libisx


@pytest.mark.parametrize("size_average", [True, False])
def test_cross_entropy_module_on_cpu_is_torchs(size_average):
    from model.custom_modules import CrossEntropyLoss
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(12, 17, generator=g) * 5).requires_grad_(True)
    y = torch.randint(0, 17, (12,), generator=g)
    zr = z.detach().clone().requires_grad_(True)
    got = CrossEntropyLoss(size_average)(z, y)
    want = nn.CrossEntropyLoss(reduction="mean" if size_average else "sum")(zr, y)
    assert got.shape == want.shape and torch.equal(got, want)
    (got * 0.75).backward()
    (want * 0.75).backward()
    assert torch.equal(z.grad, zr.grad)
    assert CrossEntropyLoss().size_average is True                                                      # the reference's default


_SPEC = "synthetic:CLICIDE_video_224sq:n=16:q=4:labels=2:size=224:struct=100"


def _finetune_cli(seed, save=None):
    """One CPU run of the entry point.  Full-batch steps (16 images, 8 of each label): the gradient of the classifier has no batch-composition
    noise, and at lr 0.3 the seeded-default-init AlexNet's loss fell from ln 2 to ~0.60 over 8 steps in every run tried, whatever the epoch order and the
    Dropout draws (which no flag seeds: every run is a new draw); lr 1 diverges after 5 steps, lr 0.05 with batches of 4 stays at ln 2."""
    cmd = [sys.executable, "-m", "train.classif_finetune", "--dataset=" + _SPEC, "--model=alexnet", "--device=-1", "--epochs=8", "--batch-size=16",
           "--loss-int=1", "--lr=0.3", "--seed=%d" % seed] + (["--save-dir=" + str(save)] if save is not None else [])
    run = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


def _losses(out):
    return [(int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in re.finditer(r"^\[(\d+), +(\d+)\] loss: (\d+\.\d{5})$", out, re.M)]


def _train_correct(out):
    return [int(c) for c, _ in re.findall(r"^TRAIN - correct: (\d+) / (\d+) - acc: ", out, re.M)]


@pytest.fixture(scope="module")
def finetuned(tmp_path_factory):
    save = tmp_path_factory.mktemp("classif")
    return _finetune_cli(1, save), save


@pytest.mark.parametrize("seed", [2, 3])
def test_fine_tuning_learns_whatever_the_seed(seed):
    """Other epoch orders, other Dropout draws: the loss still falls and the net, which scores every image as one class at the start (8 of 16),
    separates the two classes of the training set at the end."""
    out = _finetune_cli(seed)
    losses, correct = _losses(out), _train_correct(out)
    print("seed %d: mean loss per epoch %s, TRAIN correct %s" % (seed, [l for _, _, l in losses], correct))
    assert len(losses) == 8 and losses[-1][2] < losses[0][2]
    assert correct[-1] > 8      # 8 of 16 = one class for every image (balanced labels); above it both classes are told apart


def test_entry_point_trains_logs_and_checkpoints(finetuned):
    out, save = finetuned
    losses = _losses(out)
    assert [e for e, _, _ in losses] == list(range(1, 9)) and all(s == 1 for _, s, _ in losses), out
    print("mean loss per epoch:", [l for _, _, l in losses])
    assert losses[-1][2] < losses[0][2]
    correct = _train_correct(out)
    assert correct[-1] > 8                                      # 8 of 16 is what ONE class for every image scores: above it both classes are told apart
    tests = re.findall(r"^TEST - correct: (\d+) / (\d+) - acc: ([0-9.]+)$", out, re.M)
    trains = re.findall(r"^TRAIN - correct: (\d+) / (\d+) - acc: ([0-9.]+)$", out, re.M)
    assert len(tests) == 9 and len(trains) == 9                                     # upfront + one evaluation per epoch
    assert all(t == "4" for _, t, _ in tests) and all(t == "16" for _, t, _ in trains)
    assert abs(float(trains[-1][2]) - int(trains[-1][0]) / 16.0) < 1e-12
    assert "Starting classification training" in out and "Finished classification training" in out and "Testing as descriptor" in out
    files = sorted(os.listdir(str(save)))
    best = [f for f in files if f.endswith("_best_classif.pth.tar")]
    assert len(best) == 1 and all("model_classif_%d.pth.tar" % e in files for e in range(9)), files
    # both checkpoints load into get_class_net() through P.preload_net (what --preload-net sets)
    import copy
    from train import classif_finetune as cf
    saved, saved_labels = copy.copy(cf.P.__dict__), list(cf.labels)
    try:
        cf.P.cuda_device, cf.P.cnn_model = -1, "alexnet"
        cf.labels[:] = ["c000", "c001"]
        for f in (best[0], "model_classif_8.pth.tar"):
            cf.P.preload_net = os.path.join(str(save), f)
            net = cf.get_class_net()
            state = torch.load(cf.P.preload_net)
            assert set(state) == set(net.state_dict())
            assert all(torch.equal(v, state[k]) for k, v in net.state_dict().items())
            assert net.classifier[-1].out_features == 2
    finally:
        cf.P.__dict__.clear(); cf.P.__dict__.update(saved); cf.labels[:] = saved_labels


def test_checkpoint_feeds_the_siamese_training(finetuned, tmp_path):
    """Pipeline round trip: stage 1's checkpoint is what `--classif-model` of stage 3 loads."""
    _, save = finetuned
    ckpt = os.path.join(str(save), "model_classif_8.pth.tar")
    state = torch.load(ckpt)
    import copy
    from train import siamese_descriptor as sd
    saved = copy.copy(sd.P.__dict__)
    try:
        P = sd.P
        P.cuda_device, P.cnn_model, P.num_classes, P.classif_model, P.feature_dim, P.feature_size2d = -1, "alexnet", 2, ckpt, 16, (6, 6)
        net = sd.get_siamese_net()                                                  # load_state_dict is strict: a key error raises here
        trunk = {k: v for k, v in net.state_dict().items() if k.startswith("features.")}
        assert trunk and all(torch.equal(v, state[k]) for k, v in trunk.items())
    finally:
        sd.P.__dict__.clear(); sd.P.__dict__.update(saved)
    # and through the command line, one epoch of triplet training on the CPU: the frozen convolutions still hold the checkpoint's weights
    drv = ("import sys, torch\nfrom train import siamese_descriptor as sd\nfrom train import _common as TC\n"
           "torch.manual_seed(0)\nsd.P.test_upfront = False\n"
           "net, _ = TC.training_cli(sys.argv[2:], sd.P, sd.run, 'train.siamese_descriptor')\n"
           "torch.save({k: v.clone() for k, v in net.state_dict().items()}, sys.argv[1])\n")
    script = tmp_path / "drv.py"
    script.write_text(drv)
    out = str(tmp_path / "siam.pt")
    run = subprocess.run([sys.executable, str(script), out, "--dataset=synthetic:CLICIDE_video_224sq:n=6:q=2:labels=2:size=224", "--model=alexnet", "--device=-1",
                          "--epochs=1", "--batch-size=4", "--micro-batch=2", "--feature-dim=16", "--seed=3", "--classif-model=" + ckpt],
                         env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    after = torch.load(out)
    from train.params import UNTRAINED_BLOCKS
    conv_keys = [k for k in state if k.startswith("features.") and k.endswith(".weight")]
    frozen = conv_keys[:UNTRAINED_BLOCKS["alexnet"]]
    assert len(frozen) == 4 and all(torch.equal(after[k], state[k]) for k in frozen)
    assert not torch.equal(after[conv_keys[4]], state[conv_keys[4]])                # conv5 was trained on from the checkpoint


class _TinyBackbone(nn.Module):
    """A backbone with the three parts extract_layers looks for: TuneClassif wraps it like a ResNet (pool + one Linear)."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv2d(3, 4, 3, stride=2), nn.BatchNorm2d(4), nn.ReLU())
        self.feature_reduc = nn.Sequential(nn.AvgPool2d(3))
        self.classifier = nn.Sequential(nn.Linear(4, 4))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run_classif(rank, world, port, out):
    sys.path.insert(0, PKG)
    torch.set_num_threads(1)
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch.optim as optim
    import utils.train_general as tg
    from model.custom_modules import CrossEntropyLoss
    from model.siamese import TuneClassif
    from train import classif_finetune as cf
    torch.manual_seed(1000 * rank)                      # replicas start from DIFFERENT weights: train_gen broadcasts rank 0's
    net = TuneClassif(_TinyBackbone(), 4, untrained=0)
    P = cf.P
    P.cuda_device, P.train_epochs, P.train_batch_size, P.train_micro_batch, P.train_seed = -1, 1, 8, 2, 5
    P.train_loss_int, P.train_test_int, P.train_pre_proc, P.train_loss_avg, P.train_bn, P.train_annealing = 1000, 1000, True, True, False, {}
    g = torch.Generator().manual_seed(1)
    ds = [(torch.randn(3, 8, 8, generator=g), "l%d" % (i % 4), "p%d" % i) for i in range(16)]     # 16 images, batch 8: two optimizer steps
    cf.labels[:] = sorted(set(l for _, l, _ in ds))
    steps = []
    real_step = tg._Stepper.step
    tg._Stepper.step = lambda self, *a, **k: steps.append(1) or real_step(self, *a, **k)
    opt = optim.SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    cf.train_classif(net, ds, (ds[:4], ds), CrossEntropyLoss(True), opt)
    assert len(steps) == 2
    torch.save({k: v.clone() for k, v in net.state_dict().items()}, out + ".%d" % rank)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_data_parallel_classification_step_is_bit_identical_to_single_process(tmp_path):
    """gloo, world size 1 vs 2, micro-batch 2, batch 8, train_seed fixed: every parameter after two optimizer steps is the same bits."""
    single, dp = str(tmp_path / "single.pt"), str(tmp_path / "dp.pt")
    mp.spawn(_run_classif, args=(1, 0, single), nprocs=1, join=True)
    mp.spawn(_run_classif, args=(2, _free_port(), dp), nprocs=2, join=True)
    a = torch.load(single + ".0")
    torch.manual_seed(0)
    init = __import__("model.siamese", fromlist=["TuneClassif"]).TuneClassif(_TinyBackbone(), 4, untrained=0).state_dict()
    assert sum(float((a[k].float() - init[k].float()).abs().sum()) for k in a) > 1e-3          # training really changed the weights
    for r in range(2):
        b = torch.load(dp + ".%d" % r)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (r, k, float((a[k].float() - b[k].float()).abs().max()))
