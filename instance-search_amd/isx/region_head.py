"""Everything behind the trunk of RegionDescriptorNet (reference model/siamese.py:140-230) with the two losses of train/siamese_regions.py
(:139-150: triplet loss on the three region descriptors + cross-entropy over the ANCHOR's k selected windows) for ALL local micro-batches of a
training step at once, forward and backward by hand over libisx.  A leaf is one triplet; rows are leaf-major [a_0; p_0; n_0; a_1; ...], M = 3 L.

The reference (and the generic route of utils/train_general._Stepper) sends each of the k windows of each image through NormalizeL2 -> Shift ->
Linear(100352 -> D) on its own and sums the k results: acc = sum_w (W x1_w + b).  The Linear is linear: acc = W s + k b with s = sum_w x1_w, and in
the backward pass every window of an image receives the same d acc, so dW = sum_images d acc (x) s and W^T d acc is needed once per image.  The
822 MB Linear therefore runs on the M image rows -- DescriptorNet's head (isx/head.HeadEngine.linear_l2) -- behind ONE new step, gather -> L2 ->
Shift -> sum over the windows (isx_region_sum_l2_nhwc), whose backward scatters an L2 backward per window into the map
(isx_region_sum_l2_bwd_nhwc).  Mathematically the reference's result; in fp32 it differs in rounding (the sum over the windows is taken in front
of the Linear instead of behind it).  The inference path (model/siamese.RegionDescriptorNet._batched_gpu, per-window rows) is untouched: the
training forward and the epoch's mining pass agree to rounding, not to the bit.

  forward    window scores as isx/classif_head.ClassifHeadEngine forms them (isx_boxpool_s1_nhwc -> isx_head_linear_fwd_rows on the class-padded
             weight) -> isx_region_topk_nhwc -> isx_region_sum_l2_nhwc -> Linear -> + (k - 1) b (the GEMM, or the shard, adds b once) ->
             isx_l2norm_rows: descriptors (M, D).
  losses     isx_triplet_leaves on the descriptors; isx_softmax_xent_leaves on the anchors' scores at their k selected windows.
  backward   isx_l2norm_rows_bwd -> RowSink (s, d acc) -> bias / Shift gradients (column sums per leaf, times k) -> isx_head_linear_dgrad;
             classifier branch on the anchors' selected windows: isx_linear_wgrad_leaves / isx_colsum_leaves ADDED into the leaves' rows,
             isx_head_linear_dgrad -> the rows placed at their windows of a zeroed (L, Ho, Wo, K) score-gradient map -> isx_boxpool_s1_bwd_nhwc: the
             class term of the L anchors; isx_region_sum_l2_bwd_nhwc adds it last to every third image (add_every = 3).
             The ReLU mask of the last block is SuffixEngine.backward's, as for every caller.

Every kernel computes a row exactly as it would alone and the per-leaf sums run over the leaf's rows in order: a leaf's losses and flat
gradient are the same bits alone or among its siblings."""
import torch

from . import _lib, ops
from .classif_head import ClassifHeadEngine
from .head import HeadEngine


class RegionHeadEngine(object):
    def __init__(self, net):
        self.k = net.k
        self.chead = ClassifHeadEngine(net)
        self.head = HeadEngine(net)

    def built_for(self, net):
        return self.k == net.k and self.chead.built_for(net) and self.head.built_for(net)

    @staticmethod
    def applicable(net):
        """The ResNets' tail (one box pool, one 1x1 classifier) and a descriptor head the head engine takes (D % 64 == 0, F % 64 == 0), fp32 on
        the GPU.  Whether a step's maps hold at least k windows is decided per step (fits)."""
        from model.siamese import PointwiseConv
        if not (ClassifHeadEngine.applicable(net) and HeadEngine.applicable(net) and isinstance(net.classifier[0], PointwiseConv)):
            return False
        ks = net.feature_reduc[0].kernel_size
        kh, kw = tuple(ks) if isinstance(ks, tuple) else (ks, ks)
        return int(getattr(net, "k", 0)) >= 1 and net.classifier[0].weight.size(1) * kh * kw == net.feature_reduc1[2].in_features

    @property
    def lin(self):
        return self.head.lin

    def fits(self, h, w):
        """loc >= k: a shorter score map makes the reference's cls_out carry zero columns; those steps stay on the generic route."""
        kh, kw = self.chead.window()
        return h >= kh and w >= kw and (h - kh + 1) * (w - kw + 1) >= self.k

    def step(self, y_all, labels, leaves, trip, trip_scales, xent_scales, sink, flat_all, slices, shard=None, leaf_ids=None):
        """y_all: (3 leaves, C, h, w) channels-last trunk output, leaf-major; labels: (leaves) class index of the anchors; trip: the triplet
        criterion (margin, normalized); trip_scales / xent_scales: (scale_a, scale_b) of isx_triplet_leaves / isx_softmax_xent_leaves.
        Writes the head's and ADDS the classifier's per-leaf gradients into flat_all, sends the Linear's rows to `sink`.  Returns (per-leaf
        triplet loss sums, per-leaf sums of the window losses, gradient wrt y_all (channels-last), flat_idx (M, k))."""
        M, C, H, W = y_all.shape
        L, k = leaves, self.k
        kh, kw = self.chead.window()
        if L <= 0 or M != 3 * L or labels.numel() != L or not self.fits(H, W) or not ops._is_nhwc(y_all):
            raise _lib.IsxError("region engine: trunk output %s / %d labels are not %d triplets of channels-last maps with at least %d %dx%d windows"
                                % (tuple(y_all.shape), labels.numel(), L, k, kh, kw))
        Ho, Wo = H - kh + 1, W - kw + 1
        loc = Ho * Wo
        N = self.chead.cls.weight.size(0)
        # ---- forward
        prow, logits, wp = self.chead.scores(y_all)                                        # (M loc, K), (M loc, N)
        flat_idx, _ = ops.region_topk(logits.view(M, Ho, Wo, N).permute(0, 3, 1, 2), k)     # (M, k)
        s, n2 = ops.region_sum_l2_nhwc(y_all, kh, kw, flat_idx, Wo, self.head.shift.param.detach())
        d, acc, sctx = self.head.linear_l2(s, shard, leaf_ids, k=k)
        # ---- losses
        per_t, dd = ops.triplet_leaves(d, L, trip.margin, trip.normalized, trip_scales[0], trip_scales[1])
        sel = (flat_idx[0::3] + torch.arange(L, device=flat_idx.device)[:, None] * (3 * loc)).reshape(-1)     # the anchors' selected window rows
        per_x, dz = ops.softmax_xent_leaves(logits.index_select(0, sel), labels.repeat_interleave(k), L, xent_scales[0], xent_scales[1])
        # ---- backward
        g = self.head.linear_l2_backward(s, acc, dd, shard, sctx, L, sink, flat_all, slices, k=k)
        self.chead.add_grads(dz, prow.index_select(0, sel), L, flat_all, slices)
        # the class term exists for the anchors alone: an (L, Ho, Wo, C) score-gradient map, rows placed at the anchors' k windows
        at = (flat_idx[0::3] + torch.arange(L, device=flat_idx.device)[:, None] * loc).reshape(-1)
        dscore = prow.new_zeros((L * loc, C))
        dscore.index_copy_(0, at, ops.head_linear_dgrad(dz, wp))                            # distinct indices: a deterministic placement
        cls_term = ops.boxpool_s1_bwd_nhwc(dscore.view(L, Ho, Wo, C).permute(0, 3, 1, 2), H, W, kh, kw)
        dy_all = ops.region_sum_l2_bwd_nhwc(y_all, g, n2, kh, kw, flat_idx, Wo, add=cls_term, add_every=3)
        return per_t, per_x, dy_all, flat_idx
