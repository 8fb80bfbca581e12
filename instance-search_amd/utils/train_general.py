"""Batch fold driver and the generic training loop (reference utils/train_general.py): fold_batches
(:27-38), anneal (:41-48), micro/mini-batch steps with gradient accumulation (:51-74), train_gen
(:77-105), output_stats (:12-23).  Added: data-parallel execution -- with torch.distributed
initialised every rank takes the micro-batches of its subtree of each mini-batch and the gradients are
summed in a fixed tree order across the ranks (isx/dp.py), bit-identical to the single-process run."""
import random

import torch
import torch.distributed as dist
import torch.optim as optim

from model.nn_utils import set_net_train
from .general import log


def fold_batches(f, init, x, batch_size, cut_end=False, add_args={}):
    """Left fold of `f(acc, start_index, is_final, x[start:end], **add_args)` over consecutive
    batches of `x`.  batch_size <= 0: one call on the whole set.  cut_end drops a trailing
    partial batch (and then flags the last FULL batch as final)."""
    n = len(x)
    if batch_size <= 0:
        return f(init, 0, True, x, **add_args)
    acc = init
    for start in range(0, n, batch_size):
        end = min(start + batch_size, n)
        if cut_end and start + batch_size > n:
            continue
        is_final = (end > n - batch_size) if cut_end else (end == n)
        acc = f(acc, start, is_final, x[start:end], **add_args)
    return acc


def output_stats(train_type, P, test_print, test_net, net, testset_tuple, epoch, batch_count, is_final, loss, running_loss, score):
    """Running-loss line every P.train_loss_int mini-batches; evaluation every P.train_test_int (or at
    the end of the epoch when that is <= 0)."""
    every = P.train_loss_int
    running_loss = running_loss + loss              # `loss` may be a device scalar (_Stepper.step): summed where it lives, in float64
    if batch_count % every == every - 1:
        log(P, '[{0:d}, {1:5d}] loss: {2:.5f}'.format(epoch + 1, batch_count + 1, float(running_loss) / every))
        running_loss = 0.0
    t = P.train_test_int
    if (t > 0 and batch_count % t == t - 1) or (t <= 0 and is_final):
        score = test_print(train_type, P, net, testset_tuple, test_net, score, epoch + 1)
    return running_loss, score


def make_sgd(params, lr, momentum, weight_decay):
    """optim.SGD as the reference builds it (train/siamese_descriptor.py:190-191); on the GPU the FUSED implementation: one pass over
    (parameter, gradient, momentum buffer) per tensor list instead of torch's default chain of foreach kernels -- 882 MB of parameters make
    the default update 3.1 ms of a 39 ms step.  Same formula: d = g + wd p; buf = momentum buf + d; p -= lr buf."""
    params = list(params)
    fused = bool(params) and all(p.is_cuda and p.dtype == torch.float32 for p in params)
    return optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, **({"fused": True} if fused else {}))


def anneal(net, optimizer, epoch, annealing_dict):
    """At the epochs listed in annealing_dict a NEW SGD is built with lr scaled by the given factor
    (momentum buffers start afresh, as in the reference)."""
    if epoch not in annealing_dict:
        return optimizer
    g = optimizer.state_dict()['param_groups'][0]
    return make_sgd((p for p in net.parameters() if p.requires_grad), g['lr'] * annealing_dict[epoch], g['momentum'], g['weight_decay'])


# Diagnostic: set to a dict to get synchronised wall-clock seconds per phase of the training step accumulated into it (tools/bench_train.py --phases);
# None (default): no synchronisation, no timing.
PHASES = None


class _phase(object):
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if PHASES is not None:
            import time
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def __exit__(self, *exc):
        if PHASES is not None:
            import time
            torch.cuda.synchronize()
            PHASES[self.name] = PHASES.get(self.name, 0.0) + time.perf_counter() - self.t
        return False


def _dp():
    return (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)


class _Stepper(object):
    """One optimizer step = the gradients of the micro-batches of a mini-batch (reference utils/train_general.py:51-74: micro_batch_gen /
    mini_batch_gen accumulate them one after the other), summed here in the canonical TREE order of isx/dp.py: a rank runs the
    micro-batches of its subtree, TreeExchange finishes the sum across the ranks in the same order, and the descriptor head's 822 MB
    weight gradient is formed once per step from the all-gathered (x, dy) rows (RowDeferredLinear / RowSink).  The update is therefore
    bit-identical for 1, 2, 4, 8 ranks.  `P.train_grad_exchange = "allreduce"` (and world sizes that are not a power of two): sequential
    accumulation over this rank's contiguous slice + bucketed all-reduce overlapped with the last backward (dp.GradAllReducer)."""

    def __init__(self, P, net, make_batch, make_loss):
        from isx import dp
        from model.custom_modules import RowDeferredLinear
        from model.siamese import RegionHooks, TrunkHooks
        self.P, self.net, self.make_batch, self.make_loss = P, net, make_batch, make_loss
        # a net without the training step's hooks (any plain nn.Module) takes the generic per-micro-batch route; so does a net of the second
        # contract (RegionHooks: RegionDescriptorNet) whenever its one engine does not drive the whole step (_region_engine)
        self.hooked = isinstance(net, TrunkHooks)
        self.region = isinstance(net, RegionHooks)
        self._rhead_step = None                      # (engine or None,) while step() runs: _region_engine's answer for that step
        self.rank, self.world = _dp()
        mode = getattr(P, 'train_grad_exchange', 'tree')
        if mode not in ('tree', 'allreduce'):
            raise ValueError("P.train_grad_exchange must be 'tree' or 'allreduce', got %r" % (mode,))
        if mode == 'tree' and not dp.is_power_of_two(self.world):
            log(P, 'world size {0} is not a power of two: gradient exchange falls back to all-reduce (not bit-identical to one process)'.format(self.world))
            mode = 'allreduce'
        self.mode = mode
        self.deferred = [m.weight for m in net.modules() if isinstance(m, RowDeferredLinear) and m.weight.requires_grad]
        rest = [p for p in net.parameters() if p.requires_grad and not any(p is w for w in self.deferred)]
        if mode == 'tree':
            self.flat = dp.FlatGrads(rest)
            self.exchange = dp.TreeExchange() if self.world > 1 else None
        else:
            self.flat = dp.GradAllReducer(rest)
            self.exchange = None
        # The descriptor head sharded by output features (isx/shard_head.py): rank r forms and applies the update of ITS rows of the 822 MB weight
        # only.  On the GPU the single process needs no shard object (its kernels already compute the canonical sums); on the CPU it does, so
        # that 1, 2, 4, 8 processes issue the same (micro-batch, feature group) GEMMs.
        self.shards = {}
        if mode == 'tree' and getattr(P, 'train_head_shard', True):
            from isx import shard_head
            for m in net.modules():
                if isinstance(m, RowDeferredLinear) and m.weight.requires_grad and shard_head.shardable(m.weight, self.world) \
                        and (self.world > 1 or not m.weight.is_cuda):
                    self.shards[id(m.weight)] = shard_head.HeadShard(m.weight, m.bias)

    def sync_head(self):
        """All ranks' rows of a sharded head to every rank (before anything reads the whole weight: embedding pass, evaluation, checkpoint)."""
        for sh in self.shards.values():
            sh.sync()

    # -- one micro-batch ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _rows(targets, total, lo, hi):
        """Rows lo:hi of every per-item tensor among the targets (the ones with `total` rows); everything else as it is."""
        return [t[lo:hi] if torch.is_tensor(t) and t.dim() > 0 and t.size(0) == total else t for t in targets]

    def _objective(self, loss, loss2, share):
        """What a micro-batch holding `share` of the mini-batch adds to the step's objective (reference utils/train_general.py:51-74)."""
        P = self.P
        obj = loss * share if P.train_loss_avg else loss
        if loss2 is not None:
            obj = obj + P.train_loss2_alpha * (loss2 * share if P.train_loss2_avg else loss2)
        return obj

    def _leaf_scales(self, criterion, k, share):
        """For a *_leaves kernel that returns per-leaf SUMS of row losses: the (scale_a, scale_b) it multiplies the gradients by -- the criterion's
        mean over the leaf's k rows, the leaf's share of the mini-batch -- and the function that scales the sums the same way."""
        avg, loss_avg = criterion.size_average, self.P.train_loss_avg

        def rescale(per_leaf):
            if avg:
                per_leaf = per_leaf / k
            return per_leaf * share if loss_avg else per_leaf
        return (1.0 / k) if avg else 1.0, share if loss_avg else 1.0, rescale

    def _forward_backward(self, triplets, offset, mini_size, batch_args, pre, arm=False):
        if pre is not None:
            # prefix features of the whole local slice were computed in one launch (frozen trunk prefix): this micro-batch takes its rows
            feats, targets_all = pre
            n = len(triplets)
            out = self.net.forward_features(*[f[offset:offset + n] for f in feats])
            loss, loss2 = self.make_loss(out, self._rows(targets_all, feats[0].size(0), offset, offset + n))
        else:
            inputs, targets = self.make_batch(triplets, len(triplets), **batch_args)
            loss, loss2 = self.make_loss(self.net(*inputs), targets)
        obj = self._objective(loss, loss2, len(triplets) / float(mini_size))
        if arm:
            self.flat.arm()                          # all-reduce path: exchange buckets as this last backward fills them
        obj.backward()
        return obj.detach().reshape(-1)[0]           # a device scalar: the step reads the running loss back once, not per micro-batch

    def _region_engine(self):
        """The engine that drives a WHOLE step of a RegionHooks net (isx/region_head.py), or None: the generic route, bit for bit what it was.
        All or nothing, decided before any prefix is computed and from what every rank knows: the script declared its losses
        (`create_loss.region_triplet = (triplet criterion, window criterion)`), one triplet per micro-batch, tree mode, the batched route not
        switched off, and the net's engine applies (ResNet tail, a head the head engine takes, frozen BatchNorm, GPU fp32)."""
        if not self.region:
            return None
        if self._rhead_step is not None:             # inside step(): decided once, at its start
            return self._rhead_step[0]
        P = self.P
        if not (self.mode == 'tree' and P.train_micro_batch == 1 and getattr(P, 'train_suffix_batched', True)
                and getattr(P, 'train_trunk_per_minibatch', True) and getattr(self.make_loss, 'region_triplet', None) is not None):
            return None
        return self.net.region_head_engine()

    def _region_fits(self, rhead, feats):
        """From the shapes alone: three branches of one shape whose trunk output holds at least k windows (a shorter score map makes the
        reference's cls_out carry zero columns: generic route)."""
        if len(feats) != 3 or len(set(tuple(f.shape[1:]) for f in feats)) != 1:
            return False
        h, w = feats[0].shape[2], feats[0].shape[3]
        eng = self.net.suffix_engine()
        for convs, _ in (eng.layers if eng is not None else ()):
            s = convs[1].stride
            h, w = (h - 1) // s + 1, (w - 1) // s + 1
        return rhead.fits(h, w)

    def _prefix_ok(self, n_leaves):
        """May the frozen trunk prefix be computed outside the micro-batches this step?"""
        if self.region:
            return bool(n_leaves >= 1 and self._region_engine() is not None)
        return bool(self.hooked and getattr(self.P, 'train_trunk_per_minibatch', True) and n_leaves >= 1 and self.net.trunk_precomputable())

    def _precompute(self, local, n_leaves, batch_args):
        """Frozen trunk prefix: ONE batch construction for the whole local slice (same image order as micro-batch by micro-batch) and one
        prefix launch; the micro-batches then run suffix + head on their rows of the features."""
        if not self._prefix_ok(n_leaves):
            return None
        rng_state = random.getstate()
        inputs, targets = self.make_batch(local, len(local), **batch_args)
        feats = self.net.precompute_trunk(*inputs, cache=bool(getattr(self.P, 'train_prefix_cache', False)))
        if feats is None or (self.region and not self._region_fits(self._region_engine(), feats)):
            # (CPU tensors, ragged shapes, a region net's map shorter than k windows): the batch is built again per micro-batch, from the same random state
            random.setstate(rng_state)
            return None
        return feats, targets

    def _flat_all(self, L):
        return self.flat.flat.new_zeros((L, self.flat.flat.numel()))                 # one zeroed flat gradient row per leaf

    @staticmethod
    def _suffix_forward(eng, feats, offsets, k):
        """The k rows of every leaf of every branch in `feats`, leaf-major ([a_0; p_0; n_0; a_1; ...]), through the trunk suffix."""
        with _phase("suffix_forward"):
            x_all = torch.cat([f[o:o + k] for o in offsets for f in feats], 0)
            if eng is not None:
                return eng.forward(x_all)                                            # no graph: the engine's backward is driven by hand
            return x_all, None                                                       # the whole trunk is frozen: nothing to train below the head

    def _suffix_backward(self, eng, saved, dy_all, L, flat_all):
        if eng is not None:
            with _phase("suffix_backward"):
                eng.backward(saved, dy_all, leaves=L, leaf_grads=(flat_all, self.flat.slices))

    def _leaves_batched(self, eng, head, mine, offsets, mini_size, pre, sink):
        """All local micro-batches through the trainable trunk suffix (isx/suffix.py) and -- when `head` is given -- the descriptor head
        (isx/head.py) in ONE forward and ONE backward each, their gradients kept apart per micro-batch.  Every row is computed exactly as in
        a launch of its own, per-leaf sums run over the leaf's rows / pixels in order: each leaf's flat gradient is bit for bit what a pass
        over that leaf alone produces -- and what a rank of a P-rank run computes.  The loss is the training script's own callback,
        evaluated per micro-batch on its rows.  Without `head` the head runs micro-batch by micro-batch under torch autograd on its rows of
        the suffix output.  Returns (flat_all (L, total), losses)."""
        P = self.P
        feats, targets_all = pre
        nb, k, L = len(feats), len(mine[0]), len(mine)
        rows = nb * k
        share = k / float(mini_size)
        flat = self.flat.flat
        flat_all = self._flat_all(L)
        y_all, saved = self._suffix_forward(eng, feats, offsets, k)
        losses = []

        def leaf_grads(out_of, x_all):
            """The script's loss on out_of(leaf j's rows of x_all) under torch autograd, leaf by leaf: the gradient wrt x_all."""
            dx_all = torch.empty_like(x_all)
            for j in range(L):
                x = x_all[j * rows:(j + 1) * rows].detach().requires_grad_(True)
                loss, loss2 = self.make_loss(out_of(x), self._rows(targets_all, feats[0].size(0), offsets[j], offsets[j] + k))
                obj = self._objective(loss, loss2, share)
                obj.backward()
                losses.append(obj.detach().reshape(-1)[0])
                if x.grad is None:                       # a loss that does not touch this leaf's rows
                    dx_all[j * rows:(j + 1) * rows].zero_()
                else:
                    dx_all[j * rows:(j + 1) * rows].copy_(x.grad)
                if head is None:
                    self.flat.attach_all()
                    flat_all[j].copy_(flat)                                          # the head's small parameters; the suffix slots are still zero
                    flat.zero_()
            return dx_all

        with _phase("heads"):
            if head is None:
                dy_all = leaf_grads(lambda z: self.net.head_rows(z, nb), y_all)
            else:
                from model.siamese import _SplitRows
                shard = sink.shard_for(head.lin.weight) if sink is not None else None
                d_all, hctx = head.forward(y_all, shard=shard, leaf_ids=list(sink.leaf_ids) if shard is not None else None)
                trip = getattr(self.make_loss, 'triplet', None)
                if trip is not None and nb == 3 and d_all.is_cuda and getattr(P, 'train_loss_batched', True):
                    # the training script declared its loss to be THE triplet criterion on (anchor, positive, negative) and nothing else
                    # (`create_loss.triplet = criterion`): all L micro-batches in one launch (isx_triplet_leaves) -- per row the arithmetic of the
                    # criterion's own kernels, the leaf's loss = its rows' losses in row order -- instead of L x (forward, sum, backward, four copies)
                    from isx import ops
                    scale_a, scale_b, rescale = self._leaf_scales(trip, k, share)
                    per_leaf, dd = ops.triplet_leaves(d_all, L, trip.margin, trip.normalized, scale_a, scale_b)
                    losses.extend(rescale(per_leaf).unbind(0))
                else:
                    dd = leaf_grads(lambda d: _SplitRows.apply(d, nb), d_all)
                dy_all = head.backward(hctx, dd, L, sink, flat_all, self.flat.slices)
        self._suffix_backward(eng, saved, dy_all, L, flat_all)
        return flat_all, losses

    @staticmethod
    def _scales_fit(eng, chead, feats, k):
        """True when every scale's trunk output holds at least one window and a micro-batch of k images has at most the 8192 window rows
        isx_softmax_xent_leaves takes per leaf (decided from the shapes alone: the same answer on every rank)."""
        from isx.classif_head import MAX_ROWS_PER_LEAF
        kh, kw = chead.window()
        for f in feats:
            h, w = f.shape[2], f.shape[3]
            for convs, _ in (eng.layers if eng is not None else ()):
                s = convs[1].stride
                h, w = (h - 1) // s + 1, (w - 1) // s + 1
            if h < kh or w < kw or k * (h - kh + 1) * (w - kw + 1) > MAX_ROWS_PER_LEAF:
                return False
        return True

    def _classif_batched(self, eng, chead, xent, mine, offsets, mini_size, pre):
        """Classifier training whose script declared its loss to be THE cross-entropy criterion `xent` on the class scores of every branch:
        classification fine-tuning (train/classif_finetune.py, `create_loss.cross_entropy = criterion`: one branch) and sub-region classifier
        training (train/classif_regions.py, `create_loss.region_cross_entropy = criterion`: one branch PER SCALE of the local images, `pre`
        holding a prefix feature tensor of its own spatial size for each, the loss taken over every window of every scale).  Scale by scale, in
        the order of the item's scale list: all local micro-batches through the trunk suffix (isx/suffix.py), pool -> classifier ->
        cross-entropy over the windows (isx/classif_head.py) and the suffix backward, gradients kept apart per micro-batch as in
        _leaves_batched.  Scale 0 writes the leaves' flat gradient rows, every further scale a buffer of its own that is then added: a leaf's
        gradient is the fp32 SUM OF ITS SCALES' GRADIENTS IN SCALE ORDER, each of them bit for bit what a pass over that leaf alone produces --
        and what a rank of a P-rank run computes.  A leaf's loss is summed over the scales the same way.  Returns (flat_all (L, total), losses)."""
        feats, targets_all = pre
        k, L, S = len(mine[0]), len(mine), len(feats)
        flat_all = self._flat_all(L)
        labels = torch.cat([targets_all[0][o:o + k] for o in offsets], 0)
        total = None
        for s, f in enumerate(feats):
            part = flat_all if s == 0 else torch.zeros_like(flat_all)
            y_all, saved = self._suffix_forward(eng, (f,), offsets, k)
            # the leaf's window rows at this scale; its share of the mini-batch, the scales averaged
            scale_a, scale_b, rescale = self._leaf_scales(xent, k * chead.rows_per_image(y_all.shape[2], y_all.shape[3]), k / float(mini_size) / S)
            with _phase("heads"):
                per_leaf, dy_all = chead.step(y_all, labels, L, scale_a, scale_b, part, self.flat.slices, need_dy=eng is not None)
                total = rescale(per_leaf) if total is None else total + rescale(per_leaf)
            self._suffix_backward(eng, saved, dy_all, L, part)
            if s > 0:
                flat_all += part
        return flat_all, list(total.unbind(0))

    def _regions_batched(self, eng, rhead, mini_size, pre, sink, mine, offsets):
        """Region-descriptor siamese training whose script declared its losses (train/siamese_regions.py, `create_loss.region_triplet =
        (criterion, criterion2)`: the triplet criterion on the three region descriptors + criterion2 over the ANCHOR's k selected windows,
        reference :139-150), one triplet per leaf: all local leaves through the trunk suffix (isx/suffix.py), everything behind it with both
        losses (isx/region_head.py) and the suffix backward, gradients kept apart per leaf as in _leaves_batched.  A leaf's loss is _objective's
        formula on its two per-leaf sums.  Returns (flat_all (L, total), losses)."""
        P = self.P
        feats, targets_all = pre
        L = len(mine)
        share = 1.0 / float(mini_size)
        trip, xent = self.make_loss.region_triplet
        k = rhead.k
        flat_all = self._flat_all(L)
        y_all, saved = self._suffix_forward(eng, feats, offsets, 1)
        labels = torch.cat([targets_all[0][o:o + 1] for o in offsets], 0)
        with _phase("heads"):
            scale_a, scale_b, rescale = self._leaf_scales(trip, 1, share)
            mean2 = xent.reduction == 'mean'
            shard = sink.shard_for(rhead.lin.weight) if sink is not None else None
            per_t, per_x, dy_all, _ = rhead.step(y_all, labels, L, trip, (scale_a, scale_b),
                                                 ((1.0 / k) if mean2 else 1.0, P.train_loss2_alpha * (share if P.train_loss2_avg else 1.0)),
                                                 sink, flat_all, self.flat.slices, shard=shard,
                                                 leaf_ids=list(sink.leaf_ids) if shard is not None else None)
            loss2 = per_x / k if mean2 else per_x
            losses = rescale(per_t) + P.train_loss2_alpha * (loss2 * share if P.train_loss2_avg else loss2)
        self._suffix_backward(eng, saved, dy_all, L, flat_all)
        return flat_all, list(losses.unbind(0))

    def _route(self, mine, n, mb, pre, sink):
        """The batched route of this step: a callable (leaves, their row offsets) -> (flat_all: one flat gradient row per leaf, losses), or
        None for the generic route (one _forward_backward per micro-batch)."""
        # batched engines need equal micro-batches; decided from the MINI-BATCH (n % mb == 0: every leaf of every rank has mb triplets), not from
        # this rank's leaves, so that every rank and the single-process run take the same numeric path (round-4 ADVICE)
        if self.region:
            # all or nothing: `pre` exists only where _region_engine and _region_fits said yes (_prefix_ok, _precompute)
            rhead = self._region_engine() if (pre is not None and mine) else None
            if rhead is None:
                return None
            import functools
            return functools.partial(self._regions_batched, self.net.suffix_engine(), rhead, n, pre, sink)
        if not (self.hooked and self.mode == 'tree' and pre is not None and mine and n % mb == 0):
            return None
        # a net whose branches are the SCALES of an image (TuneClassifSub: feature maps of different size per branch) takes the
        # classifier route or the generic one, never _leaves_batched (which stacks the branches)
        scales = self.net.branches_are_scales
        xent = getattr(self.make_loss, 'region_cross_entropy' if scales else 'cross_entropy', None)
        chead = self.net.classif_head_engine() if xent is not None else None
        if chead is None and scales:
            return None
        eng, head = self.net.suffix_engine(), self.net.head_engine()
        if chead is not None and self._scales_fit(eng, chead, pre[0], mb):
            return lambda m, o: self._classif_batched(eng, chead, xent, m, o, n, pre)
        if not scales and (eng is not None or head is not None):
            return lambda m, o: self._leaves_batched(eng, head, m, o, n, pre, sink)
        return None

    def _slice(self, mini_batch):
        """This rank's micro-batches of a mini-batch: (leaves, first leaf index, one past the last, their items in order, row offset of each leaf)."""
        from isx import dp
        P, n = self.P, len(mini_batch)
        mb = P.train_micro_batch if 0 < P.train_micro_batch < n else n
        if self.mode == 'tree':
            leaves = [mini_batch[s:s + mb] for s in range(0, n, mb)]
            lo, hi = dp.rank_leaves(len(leaves), self.world, self.rank)
            mine = leaves[lo:hi]
        else:
            sl = mini_batch[(n * self.rank) // self.world:(n * (self.rank + 1)) // self.world]
            mine = [sl[s:s + mb] for s in range(0, len(sl), mb)]
            lo, hi = 0, len(mine)
        local = [t for leaf in mine for t in leaf]
        offsets = [sum(len(l) for l in mine[:j]) for j in range(len(mine))]
        return mine, lo, hi, local, offsets

    def begin_epoch(self, dataset, batch_args):
        """The epoch's item list, for the prefix look-ahead of _precompute_ahead (None: every step computes its own prefix)."""
        self._epoch_set, self._ahead = dataset, None

    def _precompute_ahead(self, start, n, n_leaves, batch_args):
        """Frozen trunk prefix for SEVERAL consecutive mini-batches in one launch (P.train_prefix_ahead of them, default 8).  The prefix of an
        image depends neither on the batch it rides in nor -- being frozen -- on the optimizer steps in between, so the features a step reads are
        bit for bit the ones its own launch would produce; 192 images fill the chip to 0.67 of the fp32 peak on these layers, 768 to 0.8.  Only
        when the training script declares its batch construction deterministic (`create_batch.deterministic`: no random augmentation, negatives
        drawn per epoch) -- the mini-batches further down the list are built ahead of their turn."""
        P = self.P
        # P.train_prefix_ahead counts mini-batches of ONE process; a rank of a P-rank run holds 1/P of each, so it looks P times further ahead:
        # the launch carries the same number of images whatever the world size (each rank decides for itself: no collective is involved)
        G = int(getattr(P, 'train_prefix_ahead', 8))
        G = G * self.world if G > 1 else G
        ds = getattr(self, '_epoch_set', None)
        if (G < 2 or ds is None or start is None or not getattr(self.make_batch, 'deterministic', False)
                or getattr(P, 'train_prefix_cache', False) or not self._prefix_ok(n_leaves)):
            return None
        a = self._ahead
        if a is None or not (a[0] <= start < a[0] + a[1] * n) or (start - a[0]) % n:
            groups, s_ = [], start
            while len(groups) < G and s_ + n <= len(ds):
                groups.append(self._slice(ds[s_:s_ + n])[3])
                s_ += n
            if len(groups) < 2 or len(set(len(g) for g in groups)) != 1 or not groups[0]:
                self._ahead = None
                return None
            items = [t for g in groups for t in g]
            inputs, targets = self.make_batch(items, len(items), **batch_args)
            feats = self.net.precompute_trunk(*inputs)
            if feats is None or (self.region and not self._region_fits(self._region_engine(), feats)):
                self._epoch_set = None           # CPU tensors / ragged shapes / too short a map for a region net: the steps build their own batches
                return None
            a = self._ahead = (start, len(groups), len(groups[0]), feats, targets, len(items))
        g, m = (start - a[0]) // n, a[2]
        feats = tuple(f[g * m:(g + 1) * m] for f in a[3])
        targets = self._rows(a[4], a[5], g * m, (g + 1) * m)
        if g == a[1] - 1:
            self._ahead = None                   # last user: the block is freed with this step
        return feats, targets

    def step(self, optimizer, mini_batch, batch_args, start=None):
        # the route of a region net is decided ONCE per step (the engine's gate walks every prefix parameter): the look-ahead, the prefix and
        # the route below all read this answer
        self._rhead_step = (self._region_engine(),) if self.region else None
        try:
            return self._step(optimizer, mini_batch, batch_args, start)
        finally:
            self._rhead_step = None

    def _step(self, optimizer, mini_batch, batch_args, start):
        from isx import dp
        P, n = self.P, len(mini_batch)
        mb = P.train_micro_batch if 0 < P.train_micro_batch < n else n
        mine, lo, hi, local, offsets = self._slice(mini_batch)
        with _phase("batch+prefix"):
            pre = self._precompute_ahead(start, n, len(mine), batch_args) if mine else None
            if pre is None:
                pre = self._precompute(local, len(mine), batch_args) if mine else None
        self.flat.zero_grad()
        losses = []
        fuse = optimizer if getattr(P, 'train_fused_head_sgd', True) else None       # head weight: gradient + SGD update as one kernel (isx/dp.py)
        # sharded head this step?  decided from what EVERY rank knows (mini-batch size, micro-batch size, world): equal micro-batches, the same
        # number on every rank (GPU) / a multiple of the 8 feature groups' rank counts (CPU: one rule for every world size, see __init__)
        n_leaves = -(-n // mb)
        shard_ok = bool(self.shards) and n % mb == 0 and self.mode == 'tree' and n_leaves % (self.world if next(iter(self.shards.values())).weight.is_cuda else 8) == 0
        if self.shards and not shard_ok:
            self.sync_head()                          # the replicated path below reads and updates the whole weight
        with dp.RowSink(self.deferred, optimizer=(optimizer if shard_ok else fuse), shards=(self.shards if shard_ok else None)) as sink:
            for sh in sink.shards.values():
                sh.begin_step(len(mine))
            sink.leaf_ids = list(range(lo, hi))
            batched = getattr(P, 'train_suffix_batched', True)
            route = self._route(mine, n, mb, pre, sink) if batched else None
            flat_all = None
            if route is not None and batched == "leaf":  # test mode: the same machinery one micro-batch at a time (what a rank with ONE leaf runs)
                parts = [route([mine[j]], [offsets[j]]) for j in range(len(mine))]
                flat_all = torch.cat([p[0] for p in parts], 0)
                losses = [l for p in parts for l in p[1]]
            elif route is not None:
                flat_all, losses = route(mine, offsets)
            if self.mode == 'tree':
                def leaf(i):
                    sink.leaf_ids = [i]
                    losses.append(self._forward_backward(mine[i - lo], offsets[i - lo], n, batch_args, pre))
                    return self.flat.take()
                if flat_all is not None and flat_all.is_cuda and 1 <= hi - lo <= 16:
                    from isx import ops
                    self.flat.attach_all()
                    ops.tree_sum_rows(flat_all, out=self.flat.flat)       # the same tree, one pass over the leaves' rows instead of L - 1 add passes
                else:
                    self.flat.put(dp.tree_sum(lo, hi, leaf if flat_all is None else (lambda i: flat_all[i - lo])))
                if self.exchange is not None:
                    self.exchange.allreduce_(self.flat.flat)
            else:
                for j, triplets in enumerate(mine):
                    losses.append(self._forward_backward(triplets, offsets[j], n, batch_args, pre, arm=(j == len(mine) - 1)))
                self.flat.finish()
            with _phase("head_weight_gradient"):
                sink.finish()
        loss = torch.stack(losses).double().sum() if losses else torch.zeros((), dtype=torch.float64)
        if self.world > 1:
            t = loss.reshape(1).to(next(self.net.parameters()).device)
            dist.all_reduce(t)
            loss = t
        with _phase("optimizer"):
            optimizer.step()
        # the loss stays a tensor (float64 scalar, on the device of the step): output_stats adds it to the running loss there and reads that back
        # when a line is printed (every P.train_loss_int steps) -- a read-back per step would leave the GPU idle while the host prepares the next
        loss = loss.reshape(())
        if self.world > 1:
            # BatchNorm in training mode (P.train_bn): each rank's running statistics saw only its slice -- average them so that the
            # replicas stay one model (same mining, same evaluation, a checkpoint that is every rank's)
            from isx.dp import average_buffers, batch_norm_buffers
            average_buffers(batch_norm_buffers(self.net))
        return loss


def train_gen(train_type, P, test_print, test_net, net, train_set, testset_tuple, optimizer, create_epoch, create_batch, create_loss,
              best_score=0):
    """Generic training driver (reference utils/train_general.py:77-105): per epoch anneal -> create_epoch ->
    mini-batches of P.train_batch_size (a trailing partial one is dropped) -> statistics / evaluation."""
    set_net_train(net, True, bn_train=P.train_bn)
    rank, world = _dp()
    if world > 1:
        from isx.dp import broadcast_module_state
        broadcast_module_state(net, src=0)      # replicas start from rank 0's weights and buffers (the descriptor head is random-init)
    stepper = _Stepper(P, net, create_batch, create_loss)
    for epoch in range(P.train_epochs):
        optimizer = anneal(net, optimizer, epoch, P.train_annealing)
        if world > 1 or getattr(P, 'train_seed', None) is not None:
            # identical couple order (and random fall-back negatives) on every rank -- and, with P.train_seed set, in a single process,
            # so that runs with 1, 2, 4, 8 ranks train on the same triplets (the reference leaves `random` unseeded)
            random.seed((getattr(P, 'train_seed', 0) or 0) + epoch)
        stepper.sync_head()                     # the epoch's embedding pass reads the whole head
        dataset, batch_args = create_epoch(epoch, train_set, testset_tuple)
        stepper.begin_epoch(dataset, batch_args)

        def one(state, start, is_final, mini_batch):
            count, score, running = state
            loss = stepper.step(optimizer, mini_batch, batch_args, start=start)
            t = P.train_test_int
            if (t > 0 and count % t == t - 1) or (t <= 0 and is_final):
                stepper.sync_head()             # output_stats evaluates the net now
            running, score = output_stats(train_type, P, test_print, test_net, net, testset_tuple, epoch, count, is_final, loss,
                                          running, score)
            return count + 1, score, running

        _, best_score, _ = fold_batches(one, (0, best_score, 0.0), dataset, P.train_batch_size, cut_end=True)
    stepper.sync_head()
    return best_score
