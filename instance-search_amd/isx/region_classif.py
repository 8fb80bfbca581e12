"""The classifier tail of TuneClassifSub (reference model/siamese.py:57-89: AvgPool2d(feature_size2d, stride=1) -> the classifier Linear as a
1x1 convolution: one class-score vector per window of the feature map) and the sub-region loss of train/classif_regions.py:80-98 (every
window of an image is a row carrying the image's label) for ALL local micro-batches of ONE scale of a training step, forward and backward by
hand over libisx.  The generalisation of isx/classif_head.ClassifHeadEngine to a window smaller than the map:

  forward    isx_boxpool_s1_nhwc (the pooling kernel of the inference path) -> the (M Ho Wo, K) window rows -> isx_head_linear_fwd_rows on the
             class-padded weight -> isx_softmax_xent_leaves with k = (M / leaves) Ho Wo rows per leaf, the image's label repeated per window.
  backward   isx_linear_wgrad_leaves + isx_colsum_leaves (classifier gradients PER micro-batch) -> isx_head_linear_dgrad ->
             isx_boxpool_s1_bwd_nhwc: gradient wrt the trunk output.  The ReLU mask of the last block is applied by SuffixEngine.backward.

The scales of an image have different spatial sizes, so a step calls `step` once per scale; the classifier's gradients are ADDED into the
leaves' rows of the flat gradient buffers (the caller zeroes them and walks the scales in a fixed order).  Every kernel computes a row exactly as
it would alone and the per-leaf sums run over the leaf's rows in order: a leaf's loss and gradients do not depend on its siblings.
"""
import torch

from . import _lib, ops
from ._lib import check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


MAX_ROWS_PER_LEAF = 8192          # isx_softmax_xent_leaves keeps a leaf's row losses in LDS


class RegionClassifEngine(object):
    def __init__(self, net):
        self.pool = net.feature_reduc[0]
        self.conv = net.classifier[0]

    @staticmethod
    def applicable(net):
        """One stride-1 average pool without padding in front of exactly one fp32 CUDA 1x1 PointwiseConv (the ResNets).  AlexNet's three-layer
        classifier (first layer a 6x6 convolution, Dropout) is not."""
        from model.siamese import BoxPool, PointwiseConv
        reduc, cls = getattr(net, "feature_reduc", None), getattr(net, "classifier", None)
        if reduc is None or cls is None or len(reduc) != 1 or len(cls) != 1:
            return False
        pool, conv = reduc[0], cls[0]
        if not isinstance(pool, BoxPool) or not isinstance(conv, PointwiseConv):
            return False
        if pool.padding not in (0, (0, 0)) or pool.ceil_mode or pool.stride not in (1, (1, 1)):
            return False
        if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding != (0, 0) or conv.dilation != (1, 1) or conv.groups != 1:
            return False
        w = conv.weight
        return w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and conv.in_channels % 64 == 0

    def window(self):
        ks = self.pool.kernel_size
        return tuple(ks) if isinstance(ks, tuple) else (ks, ks)

    def rows_per_image(self, h, w):
        kh, kw = self.window()
        return (h - kh + 1) * (w - kw + 1)

    def _padded(self):
        """(weight (Np, K), bias (Np)) zero-padded to a multiple of 64 classes, kept on the module and rebuilt when its parameters change."""
        from model.nn_utils import _derived
        conv = self.conv
        N, K = conv.out_channels, conv.in_channels
        if N % 64 == 0:
            return conv.weight.detach().view(N, K), (conv.bias.detach() if conv.bias is not None else None)
        return _derived(conv, '_c_pad64', (conv.weight,) + ((conv.bias,) if conv.bias is not None else ()),
                        lambda: ops.pad_rows_to_64(conv.weight.detach().view(N, K), conv.bias))

    def step(self, y_all, labels, leaves, scale_a, scale_b, flat_all, slices, need_dy=True):
        """y_all: (M, K, h, w) channels-last trunk output of `leaves` consecutive micro-batches of equal image count, ONE scale (no graph);
        labels: (M) class index per image.  ADDS the classifier's per-leaf gradients into row l of flat_all at the parameters' slices.  Returns
        (per-leaf sum of the row losses (leaves,), gradient wrt y_all (channels-last) or None when need_dy is False), gradients scaled by
        scale_a * scale_b."""
        M, Cc, H, W = y_all.shape
        conv = self.conv
        N, K = conv.out_channels, conv.in_channels
        kh, kw = self.window()
        if leaves <= 0 or M % leaves or Cc != K or H < kh or W < kw or labels.numel() != M:
            raise _lib.IsxError("region classifier engine: trunk output %s / %d labels are not %d equal micro-batches of (%d, h, w) maps of at least %dx%d"
                                % (tuple(y_all.shape), labels.numel(), leaves, K, kh, kw))
        Ho, Wo = H - kh + 1, W - kw + 1
        loc = Ho * Wo
        R = (M // leaves) * loc
        if R > MAX_ROWS_PER_LEAF:
            raise _lib.IsxError("region classifier engine: %d window rows per micro-batch (at most %d)" % (R, MAX_ROWS_PER_LEAF))
        pooled = ops.boxpool_s1_nhwc(y_all, kh, kw) if ops.boxpool_s1_applicable_nhwc(y_all) else ops.boxpool_s1(y_all.float(), kh, kw)
        rows = pooled.permute(0, 2, 3, 1).reshape(M * loc, K)                  # a view of the channels-last result: image-major, then window
        if not rows.is_contiguous():
            rows = rows.contiguous()
        wp, bp = self._padded()
        Np = wp.size(0)
        logits = ops.head_linear(rows, wp, bp)
        if Np != N:
            logits = logits[:, :N].contiguous()
        row_labels = labels.repeat_interleave(loc)
        per_leaf, dz = ops.softmax_xent_leaves(logits, row_labels, leaves, scale_a, scale_b)
        if conv.weight.requires_grad:
            lo, hi = slices[conv.weight]
            flat_all[:, lo:hi] += ops.linear_wgrad_leaves(dz, rows, leaves).view(leaves, -1)
        if conv.bias is not None and conv.bias.requires_grad:
            gb = torch.empty((leaves, N), dtype=torch.float32, device=dz.device)
            check(lib().isx_colsum_leaves(dz.data_ptr(), leaves, R, N, gb.data_ptr(), _stream()), "isx_colsum_leaves")
            lo, hi = slices[conv.bias]
            flat_all[:, lo:hi] += gb
        if not need_dy:
            return per_leaf, None
        Mr = M * loc
        Mp = (Mr + 63) // 64 * 64
        dzT = dz.new_zeros((Np, Mp))                            # padding classes and rows: zero products leave every chain untouched
        dzT[:N, :Mr] = dz.t()
        dpool = torch.empty((Mp, K), dtype=torch.float32, device=dz.device)
        check(lib().isx_head_linear_dgrad(dzT.data_ptr(), Mp, Np, wp.data_ptr(), K, dpool.data_ptr(), _stream()), "isx_head_linear_dgrad")
        return per_leaf, ops.boxpool_s1_bwd_nhwc(dpool[:Mr].view(M, Ho, Wo, K).permute(0, 3, 1, 2), H, W, kh, kw)
