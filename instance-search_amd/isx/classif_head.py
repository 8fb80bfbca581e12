"""The classifier tail of TuneClassif (reference model/siamese.py:20-32: AvgPool2d over the whole map -> Linear(2048 -> num_classes)) and its
cross-entropy loss (train/classif_finetune.py:154) for ALL local micro-batches of a classification fine-tuning step at once, forward and
backward by hand over libisx.

torch (and the reference, utils/train_general.py:51-74) run the tail once per micro-batch: pool, Linear, log-softmax, NLL, their four
backward nodes, two gradient accumulations -- ~20 launches on tensors of 8 x 464 floats, per micro-batch.  Here every local row goes through
ONE pass:

  (torch still moves small tensors in between: the class scores are cut out of the padded GEMM output, dz is transposed + zero-padded for the
  dgrad kernel, and the per-leaf weight gradients are copied from the kernel's contiguous (L, N, K) result into the leaves' rows of the flat
  gradient buffers -- 3.8 MB per leaf.)

  forward    isx_boxpool_s1_nhwc (the pooling kernel of the inference path: same means) -> isx_head_linear_fwd_rows (class dimension
             zero-padded to the GEMM's granule, as model/siamese._linear_rows does for inference: same scores) -> isx_softmax_xent_leaves
             (loss per micro-batch + gradient wrt the scores).
  backward   isx_linear_wgrad_leaves (weight gradient PER micro-batch, one row-ordered fma chain per element) -> isx_colsum_leaves (bias
             gradient per micro-batch) -> isx_head_linear_dgrad -> isx_gap_bwd_nhwc: gradient wrt the trunk output.  The ReLU mask of the
             last block is NOT fused here: SuffixEngine.backward applies it (isx_relu_grad) as for every other caller.

Every kernel computes a row exactly as it would alone and the per-micro-batch sums run over that micro-batch's rows in order, so the loss and
the gradients of a micro-batch are the same bits whether 1 or 8 micro-batches share the pass (isx/dp.py's canonical tree needs just that).
The 3.8 MB weight gets an ordinary per-leaf gradient in the step's flat buffers: nothing is deferred to a RowSink.
"""
import torch

from . import _lib, ops
from ._lib import check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class ClassifHeadEngine(object):
    def __init__(self, net):
        self.pool = net.feature_reduc[0]
        self.lin = net.classifier[0]

    @staticmethod
    def applicable(net):
        """A single fp32 CUDA Linear behind a single average pool (the ResNets).  AlexNet's three-Linear classifier with Dropout is not."""
        reduc, cls = getattr(net, "feature_reduc", None), getattr(net, "classifier", None)
        if reduc is None or cls is None or len(reduc) != 1 or len(cls) != 1:
            return False
        pool, lin = reduc[0], cls[0]
        if not isinstance(pool, torch.nn.AvgPool2d) or not isinstance(lin, torch.nn.Linear):
            return False
        if pool.padding not in (0, (0, 0)) or pool.ceil_mode:
            return False
        w = lin.weight
        return w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and lin.in_features % 64 == 0

    def _whole_map(self, y):
        ks = self.pool.kernel_size
        ks = ks if isinstance(ks, tuple) else (ks, ks)
        return tuple(y.shape[2:]) == tuple(ks)

    def _padded(self):
        """(weight, bias) zero-padded to a multiple of 64 classes: the copy RowsLinear keeps for inference (rebuilt when the weight changes)."""
        from model.nn_utils import _derived
        lin = self.lin
        if lin.out_features % 64 == 0:
            return lin.weight.detach(), (lin.bias.detach() if lin.bias is not None else None)
        return _derived(lin, '_c_pad64', (lin.weight,) + ((lin.bias,) if lin.bias is not None else ()), lambda: ops.pad_rows_to_64(lin.weight, lin.bias))

    def step(self, y_all, labels, leaves, scale_a, scale_b, flat_all, slices, need_dy=True):
        """y_all: (M, C, h, w) channels-last trunk output of `leaves` consecutive micro-batches of equal row count (no graph); labels: (M) class
        indices.  Writes the classifier's per-leaf gradients into row l of flat_all at the parameters' slices.  Returns (per-leaf sum of the row
        losses (leaves,), gradient wrt y_all (channels-last) or None when need_dy is False), gradients scaled by scale_a * scale_b."""
        M, Cc, H, W = y_all.shape
        lin = self.lin
        N, K = lin.out_features, lin.in_features
        if M % leaves or Cc != K or not self._whole_map(y_all):
            raise _lib.IsxError("classifier engine: trunk output %s is not %d equal micro-batches of (%d, h, w) maps spanned by the pool"
                                % (tuple(y_all.shape), leaves, K))
        R = M // leaves
        pooled = (ops.boxpool_s1_nhwc(y_all, H, W) if ops.boxpool_s1_applicable_nhwc(y_all) else ops.boxpool_s1(y_all.float(), H, W)).reshape(M, K)
        wp, bp = self._padded()
        Np = wp.size(0)
        logits = ops.head_linear(pooled, wp, bp)
        if Np != N:
            logits = logits[:, :N].contiguous()
        per_leaf, dz = ops.softmax_xent_leaves(logits, labels, leaves, scale_a, scale_b)
        if lin.weight.requires_grad:
            lo, hi = slices[lin.weight]
            flat_all[:, lo:hi].copy_(ops.linear_wgrad_leaves(dz, pooled, leaves).view(leaves, -1))
        if lin.bias is not None and lin.bias.requires_grad:
            gb = torch.empty((leaves, N), dtype=torch.float32, device=dz.device)
            check(lib().isx_colsum_leaves(dz.data_ptr(), leaves, R, N, gb.data_ptr(), _stream()), "isx_colsum_leaves")
            lo, hi = slices[lin.bias]
            flat_all[:, lo:hi].copy_(gb)
        if not need_dy:
            return per_leaf, None
        Mp = (M + 63) // 64 * 64
        dzT = dz.new_zeros((Np, Mp))                            # padding classes and rows: zero products leave every chain untouched
        dzT[:N, :M] = dz.t()
        dpool = torch.empty((Mp, K), dtype=torch.float32, device=dz.device)
        check(lib().isx_head_linear_dgrad(dzT.data_ptr(), Mp, Np, wp.data_ptr(), K, dpool.data_ptr(), _stream()), "isx_head_linear_dgrad")
        return per_leaf, ops.gap_bwd_nhwc(dpool[:M], H, W)
