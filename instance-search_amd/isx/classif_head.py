"""The classifier tail of TuneClassif (reference model/siamese.py:20-32: AvgPool2d over the whole map -> Linear(2048 -> num_classes)) and of
TuneClassifSub (reference model/siamese.py:57-89: AvgPool2d(feature_size2d, stride=1) -> the classifier Linear as a 1x1 convolution: one
class-score vector per window of the feature map) with their cross-entropy losses (train/classif_finetune.py:154; train/classif_regions.py:80-98:
every window of an image is a row carrying the image's label) for ALL local micro-batches of a training step at once -- of ONE scale of it for
TuneClassifSub, whose scales differ in spatial size -- forward and backward by hand over libisx.

torch (and the reference, utils/train_general.py:51-74) run the tail once per micro-batch: pool, Linear, log-softmax, NLL, their four
backward nodes, two gradient accumulations -- ~20 launches on tensors of 8 x 464 floats, per micro-batch.  Here every local row goes through
ONE pass:

  (torch still moves small tensors in between: the class scores are cut out of the padded GEMM output, dz is transposed + zero-padded for the
  dgrad kernel, and the per-leaf weight gradients are added from the kernel's contiguous (L, N, K) result into the leaves' rows of the flat
  gradient buffers -- 3.8 MB per leaf.)

  forward    isx_boxpool_s1_nhwc (the pooling kernel of the inference path: same means) -> the (M Ho Wo, K) window rows, image-major (Ho = Wo =
             1: one row per image) -> isx_head_linear_fwd_rows (class dimension zero-padded to the GEMM's granule, as
             model/siamese._linear_rows does for inference: same scores) -> isx_softmax_xent_leaves with (M / leaves) Ho Wo rows per leaf, the
             image's label repeated per window (loss per micro-batch + gradient wrt the scores).
  backward   isx_linear_wgrad_leaves (weight gradient PER micro-batch, one row-ordered fma chain per element) -> isx_colsum_leaves (bias
             gradient per micro-batch) -> isx_head_linear_dgrad -> isx_gap_bwd_nhwc (a window spanning the map) or isx_boxpool_s1_bwd_nhwc (any
             other): gradient wrt the trunk output.  The ReLU mask of the last block is NOT fused here: SuffixEngine.backward applies it
             (isx_relu_grad) as for every other caller.

Every kernel computes a row exactly as it would alone and the per-micro-batch sums run over that micro-batch's rows in order, so the loss and
the gradients of a micro-batch are the same bits whether 1 or 8 micro-batches share the pass (isx/dp.py's canonical tree needs just that).
The classifier's gradients are ADDED into the leaves' rows of the step's flat buffers (the caller zeroes them and walks the scales in a fixed
order); the 3.8 MB weight gets an ordinary per-leaf gradient there: nothing is deferred to a RowSink.
"""
import torch

from . import _lib, ops

MAX_ROWS_PER_LEAF = 8192          # isx_softmax_xent_leaves keeps a leaf's row losses in LDS


class ClassifHeadEngine(object):
    def __init__(self, net):
        self.pool = net.feature_reduc[0]
        self.cls = net.classifier[0]                   # nn.Linear (N, K) or 1x1 PointwiseConv (N, K, 1, 1): the same (N, K) matrix

    def built_for(self, net):
        return self.cls is net.classifier[0] and self.pool is net.feature_reduc[0]

    @staticmethod
    def applicable(net):
        """One average pool without padding in front of exactly one fp32 CUDA classifier (the ResNets): an nn.Linear, or a 1x1 PointwiseConv
        behind a stride-1 BoxPool.  AlexNet's three-layer classifier (Dropout; as convolutions the first one 6x6) is not."""
        from model.siamese import BoxPool, PointwiseConv
        reduc, cls = getattr(net, "feature_reduc", None), getattr(net, "classifier", None)
        if reduc is None or cls is None or len(reduc) != 1 or len(cls) != 1:
            return False
        pool, cls = reduc[0], cls[0]
        if not isinstance(pool, torch.nn.AvgPool2d) or pool.padding not in (0, (0, 0)) or pool.ceil_mode:
            return False
        if isinstance(cls, PointwiseConv):
            if not isinstance(pool, BoxPool) or pool.stride not in (1, (1, 1)):
                return False
            if cls.kernel_size != (1, 1) or cls.stride != (1, 1) or cls.padding != (0, 0) or cls.dilation != (1, 1) or cls.groups != 1:
                return False
        elif not isinstance(cls, torch.nn.Linear):
            return False
        w = cls.weight
        return w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.size(1) % 64 == 0

    def window(self):
        ks = self.pool.kernel_size
        return tuple(ks) if isinstance(ks, tuple) else (ks, ks)

    def rows_per_image(self, h, w):
        kh, kw = self.window()
        return (h - kh + 1) * (w - kw + 1)

    def _padded(self):
        """(weight (Np, K), bias (Np)) zero-padded to a multiple of 64 classes: the copy RowsLinear keeps for inference, on the module and rebuilt
        when its parameters change."""
        from model.nn_utils import _derived
        cls = self.cls
        N, K = cls.weight.shape[:2]
        if N % 64 == 0:
            return cls.weight.detach().view(N, K), (cls.bias.detach() if cls.bias is not None else None)
        return _derived(cls, '_c_pad64', (cls.weight,) + ((cls.bias,) if cls.bias is not None else ()),
                        lambda: ops.pad_rows_to_64(cls.weight.detach().view(N, K), cls.bias))

    def step(self, y_all, labels, leaves, scale_a, scale_b, flat_all, slices, need_dy=True):
        """y_all: (M, K, h, w) channels-last trunk output of `leaves` consecutive micro-batches of equal image count, ONE scale (no graph);
        labels: (M) class index per image.  ADDS the classifier's per-leaf gradients into row l of flat_all at the parameters' slices.  Returns
        (per-leaf sum of the row losses (leaves,), gradient wrt y_all (channels-last) or None when need_dy is False), gradients scaled by
        scale_a * scale_b."""
        M, Cc, H, W = y_all.shape
        cls = self.cls
        N, K = cls.weight.shape[:2]
        kh, kw = self.window()
        if leaves <= 0 or M % leaves or Cc != K or H < kh or W < kw or labels.numel() != M:
            raise _lib.IsxError("classifier engine: trunk output %s / %d labels are not %d equal micro-batches of (%d, h, w) maps of at least %dx%d"
                                % (tuple(y_all.shape), labels.numel(), leaves, K, kh, kw))
        if isinstance(cls, torch.nn.Linear) and (H, W) != (kh, kw):           # a Linear has one row of scores per image
            raise _lib.IsxError("classifier engine: trunk output %s is not %d equal micro-batches of (%d, h, w) maps spanned by the pool"
                                % (tuple(y_all.shape), leaves, K))
        Ho, Wo = H - kh + 1, W - kw + 1
        loc = Ho * Wo
        R = (M // leaves) * loc
        if R > MAX_ROWS_PER_LEAF:
            raise _lib.IsxError("classifier engine: %d window rows per micro-batch (at most %d)" % (R, MAX_ROWS_PER_LEAF))
        rows, logits, wp = self.scores(y_all)
        per_leaf, dz = ops.softmax_xent_leaves(logits, labels if loc == 1 else labels.repeat_interleave(loc), leaves, scale_a, scale_b)
        self.add_grads(dz, rows, leaves, flat_all, slices)
        if not need_dy:
            return per_leaf, None
        dpool = ops.head_linear_dgrad(dz, wp)                   # (M loc, K); against the class-padded weight
        if loc == 1:                                            # the window spans the map: one term per pixel, the division alone
            return per_leaf, ops.gap_bwd_nhwc(dpool, H, W)
        return per_leaf, ops.boxpool_s1_bwd_nhwc(dpool.view(M, Ho, Wo, K).permute(0, 3, 1, 2), H, W, kh, kw)

    def scores(self, y_all):
        """pool -> classifier on every window of every image: (pooled window rows (M loc, K), image-major, then window; class scores (M loc, N);
        the class-padded weight the scores were formed against -- what head_linear_dgrad takes)."""
        M, K = y_all.shape[:2]
        kh, kw = self.window()
        N = self.cls.weight.size(0)
        pooled = ops.boxpool_s1_nhwc(y_all, kh, kw) if ops.boxpool_s1_applicable_nhwc(y_all) else ops.boxpool_s1(y_all.float(), kh, kw)
        rows = pooled.permute(0, 2, 3, 1).reshape(-1, K)                       # a view of the channels-last result: image-major, then window
        if not rows.is_contiguous():
            rows = rows.contiguous()
        wp, bp = self._padded()
        logits = ops.head_linear(rows, wp, bp)
        if wp.size(0) != N:
            logits = logits[:, :N].contiguous()
        return rows, logits, wp

    def add_grads(self, dz, rows, leaves, flat_all, slices):
        """ADDS the classifier's per-leaf gradients (dz: gradient wrt the scores of `rows`, equal row counts per leaf) into the leaves' rows of
        flat_all at the parameters' slices."""
        cls = self.cls
        if cls.weight.requires_grad:
            lo, hi = slices[cls.weight]
            flat_all[:, lo:hi] += ops.linear_wgrad_leaves(dz, rows, leaves).view(leaves, -1)
        if cls.bias is not None and cls.bias.requires_grad:
            lo, hi = slices[cls.bias]
            flat_all[:, lo:hi] += ops.colsum_leaves(dz, leaves)
