"""Thin torch-tensor wrappers over the C ABI (include/isx.h).  One function per entry.

All tensors must live on the GPU; work is enqueued on torch's current stream.  The product
path touches ctypes here and, for the entries they alone use, in isx/suffix.py, isx/shard_head.py and isx/dp.py.

libisx receives raw pointers: it checks shapes, only a wrapper can check a buffer's size.  Every wrapper states its contract through the
checkers below and through nothing else, in one order: first what tensor metadata decides (rank, dtype, shapes, lengths, memory layout
-- testable without a GPU), then `_cuda` (device residency), and only then are outputs allocated and libisx called."""
import torch

from . import _lib
from ._lib import check, lib

EPS = 1e-10  # model/custom_modules.py:48 NormalizeL2Fun(eps=1e-10)
ANY4 = (None, None, None, None)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    return check(getattr(lib(), name)(*args), name)


def _launch(name, *args):
    """One libisx entry, enqueued on torch's current stream (the last argument of every entry that launches)."""
    return _call(name, *args, _stream())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _on_current_device(t, name):
    """Launches go to the CURRENT device's current stream: a tensor of another GPU would be touched from the wrong
    device / stream, so it is refused (select the device with torch.cuda.device(...) around the call)."""
    if t.device.index != torch.cuda.current_device():
        raise _lib.IsxError("%s lives on %s but the current device is cuda:%d -- wrap the call in torch.cuda.device(%s)"
                            % (name, t.device, torch.cuda.current_device(), t.device.index))


def _cuda(**tensors):
    """The LAST check of every wrapper: each tensor given (None = an optional argument left out) lives on the current device.
    Returns that device, for the outputs."""
    dev = None
    for name, t in tensors.items():
        if t is not None:
            if not t.is_cuda:
                raise _lib.IsxError("%s must be a CUDA tensor (libisx has no CPU path)" % name)
            _on_current_device(t, name)
            dev = t.device
    return dev


def _meta(t, name, dtype=None, shape=None, what=None):
    """What a tensor's metadata decides.  `shape`: a tuple = that rank, None entries any size; an int = that many elements (the
    per-channel / per-row vectors: bias, shift, labels); `what`: the shape in the docstring's symbols, shown next to the numbers."""
    if not isinstance(t, torch.Tensor):
        raise _lib.IsxError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
    if dtype is not None and t.dtype != dtype:
        raise _lib.IsxError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if isinstance(shape, int):
        if t.numel() != shape:
            raise _lib.IsxError("%s has %d elements, needs %s%d" % (name, t.numel(), what + " = " if what else "", shape))
    elif shape is not None and (t.dim() != len(shape) or any(e is not None and e != s for e, s in zip(shape, t.shape))):
        need = "(%s)" % ", ".join("any" if e is None else str(e) for e in shape)
        raise _lib.IsxError("%s has shape %s, needs %s" % (name, tuple(t.shape), what + " = " + need if what else need))
    return t


def _f32(t, name, shape=None, what=None):
    """A float32 INPUT, made contiguous (a copy where it is not)."""
    return _meta(t, name, torch.float32, shape, what).contiguous()


def _typed(t, dtype, name, shape=None):
    """An INPUT of any dtype, converted to `dtype` and made contiguous."""
    return _meta(t, name, None, shape).to(dtype).contiguous()


def _out(t, shape, dtype, name):
    """A buffer of the caller's that libisx uses IN PLACE (out=, ws=, the resident image set): exactly this dtype and shape, dense.  Never
    copied or converted -- a silent copy would receive the result in the caller's place."""
    if not _meta(t, name, dtype, shape).is_contiguous():
        raise _lib.IsxError("%s must be contiguous, has strides %s for shape %s" % (name, t.stride(), tuple(t.shape)))
    return t


def _nhwc(t, name, shape=ANY4, what="(B,C,H,W)", fmt=torch.channels_last):
    """The one spelling of "float32 (B,C,H,W) tensor whose memory is dense channels-last" (fmt: another memory format).  Returns (B, C, H, W)."""
    if not _meta(t, name, torch.float32, shape, what).is_contiguous(memory_format=fmt):
        raise _lib.IsxError("%s must be dense %s memory, has strides %s for shape %s"
                            % (name, "NCHW" if fmt is torch.contiguous_format else "channels-last (NHWC)", t.stride(), tuple(t.shape)))
    return t.shape


def _residual(r, shape, fmt=torch.channels_last):
    """The residual of a fused epilogue: float32, the output's shape and memory format.  Returns its pointer, 0 for none."""
    if r is None:
        return 0
    _nhwc(r, "residual", tuple(shape), "the output's shape", fmt)
    return r.data_ptr()


def _topk_out(M, k, out=None, **inputs):
    """The (M,k) float32 score / (M,k) int64 index pair of every top-k entry: the caller's `out` pair, checked, or a new one.  Closes the
    wrapper's checks with _cuda(**inputs)."""
    if out is not None:
        out = _out(out[0], (M, k), torch.float32, "out[0]"), _out(out[1], (M, k), torch.int64, "out[1]")
        _cuda(**inputs, **{"out[0]": out[0], "out[1]": out[1]})
        return out
    dev = _cuda(**inputs)
    return torch.empty((M, k), device=dev, dtype=torch.float32), torch.empty((M, k), device=dev, dtype=torch.int64)


def l2norm_rows(x, eps=EPS, out=None):
    x = _f32(x, "x", (None, None))
    B, D = x.shape
    y = out if out is None else _out(out, (B, D), torch.float32, "out")
    _cuda(x=x, out=y)
    if y is None:
        y = torch.empty_like(x)
    _launch("isx_l2norm_rows", x.data_ptr(), B, D, eps, y.data_ptr())
    return y


def l2norm_rows_bwd(x, dy, eps=EPS):
    """Gradient of l2norm_rows wrt x: (n2 dy - x <x, dy>) / (n2 sqrt(n2)), n2 = sum x^2 + eps, per row."""
    x = _f32(x, "x", (None, None))
    dy = _f32(dy, "dy", tuple(x.shape), "x's shape")
    _cuda(x=x, dy=dy)
    B, D = x.shape
    dx = torch.empty_like(x)
    _launch("isx_l2norm_rows_bwd", x.data_ptr(), dy.data_ptr(), B, D, eps, dx.data_ptr())
    return dx


def l2norm_shift_rows(x, shift=None, eps=EPS):
    x = _f32(x, "x", (None, None))
    B, F = x.shape
    shift = shift if shift is None else _f32(shift, "shift", F)
    _cuda(x=x, shift=shift)
    y = torch.empty_like(x)
    _launch("isx_l2norm_shift_rows", x.data_ptr(), _ptr(shift), B, F, eps, y.data_ptr())
    return y


def head_linear_applicable(rows, weight, any_width=False):
    """any_width: N need not be a multiple of 64 nor K of 32 (head_linear_any pads the weight with zeros)."""
    K = weight.size(1) if weight.dim() == 2 else 0
    Kp = (K + 31) // 32 * 32 if any_width else K
    return (rows.is_cuda and rows.dtype == torch.float32 and weight.dtype == torch.float32 and weight.is_contiguous() and rows.dim() == 2
            and weight.dim() == 2 and Kp % 32 == 0 and Kp > 0 and (any_width or weight.size(0) % 64 == 0) and 192 * Kp * 4 < 2 ** 32
            and rows.size(0) < 2 ** 24)


def pad_rows_to_64(weight, bias=None):
    """(weight, bias) padded with zeros to the GEMM's granules: rows (output features) to a multiple of 64 (head_linear's tile height) and
    -- for a weight whose K is not a multiple of 32 -- columns to a multiple of 32 (the k-tile)."""
    N, K = weight.shape
    Np, Kp = (N + 63) // 64 * 64, (K + 31) // 32 * 32
    wp = weight.new_zeros((Np, Kp))
    wp[:N, :K].copy_(weight.detach())
    bp = None
    if bias is not None:
        bp = bias.new_zeros((Np,))
        bp[:N].copy_(bias.detach())
    return wp, bp


def head_linear_any(rows, weight, bias=None, padded=None):
    """head_linear for any number of output features and any K: zeros pad the weight (and the bias) to a multiple of 64 outputs and of 32
    inputs, the rows are padded with zero columns to the same K, the padding outputs are dropped.  Every output element is its own set of
    k-ordered chains, and a zero product leaves a chain's value untouched (fma(0, 0, acc) == acc), so the padding changes no value: the
    result is what the kernel would compute with a zero-filled k tail, still independent of the batch (no torch / hipBLASLt GEMM, whose
    kernel choice depends on M).  `padded`: the (weight, bias) pair of pad_rows_to_64, kept by the caller next to its weight
    (model/siamese.RowsLinear caches it per version of the parameter); None: padded here, per call.
    For the classifier layers of TuneClassif (2048 -> 464 class scores, reference model/siamese.py:28-32): a row's scores do not depend on the
    batch it is computed in, as with every other descriptor of the path."""
    N, K = weight.shape
    if N % 64 == 0 and K % 32 == 0:
        return head_linear(rows, weight, bias)
    wp, bp = padded if padded is not None else pad_rows_to_64(weight, bias)
    if wp.size(1) != K:
        rows = torch.nn.functional.pad(rows, (0, wp.size(1) - K))
    y = head_linear(rows, wp, bp)
    return y if N == wp.size(0) else y[:, :N].contiguous()


def head_linear(rows, weight, bias=None):
    """y = rows . weight^T + bias on libisx's split-K GEMM (isx_head_linear_fwd_rows): a row's result does not depend on how many rows ride along,
    and it is the same kernel the training step runs -- one implementation of DescriptorNet's Linear (reference model/siamese.py:104-122).
    rows: (M, K) fp32, weight: (N, K) as nn.Linear stores it, K % 32 == 0, N % 64 == 0."""
    rows = _f32(rows, "rows", (None, None))
    M, K = rows.shape
    weight = _f32(weight, "weight", (None, K), "(N, K)")
    N = weight.size(0)
    if K % 32 != 0 or N % 64 != 0:
        raise _lib.IsxError("head_linear: rows (%d, %d) against weight %s (K %% 32 == 0, N %% 64 == 0)" % (M, K, tuple(weight.shape)))
    bias = bias if bias is None else _f32(bias, "bias", N)
    dev = _cuda(rows=rows, weight=weight, bias=bias)
    y = torch.empty((M, N), dtype=torch.float32, device=dev)
    if M == 0:
        return y
    # the split-K workspace is a fresh allocation per call: the caching allocator keeps a stream's blocks to that stream, so two calls under
    # two current streams never share scratch memory (a workspace cached per device did)
    ws = torch.empty(lib().isx_head_linear_rows_workspace(M, K, N) // 4, dtype=torch.float32, device=dev)
    _launch("isx_head_linear_fwd_rows", rows.data_ptr(), M, K, weight.data_ptr(), N, _ptr(bias), y.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    return y


def gap_l2(fmap, eps=EPS, out=None):
    """Global average pool + L2 of a logical (B,C,H,W) feature map.  A channels-last tensor (the
    layout NHWC convolutions produce) is consumed in place by the NHWC kernel -- no transpose."""
    B, Cc, H, W = _meta(fmap, "fmap", torch.float32, ANY4, "(B,C,H,W)").shape
    y = out if out is None else _out(out, (B, Cc), torch.float32, "out")
    dev = _cuda(fmap=fmap, out=y)
    if y is None:
        y = torch.empty((B, Cc), device=dev, dtype=torch.float32)
    if _is_nhwc(fmap):
        _launch("isx_gap_l2_nhwc", fmap.data_ptr(), B, Cc, H, W, eps, y.data_ptr())
    else:
        fmap = fmap.contiguous()
        _launch("isx_gap_l2", fmap.data_ptr(), B, Cc, H, W, eps, y.data_ptr())
    return y


def bias_act_(y, bias, residual=None, relu=True):
    """In place y = act(y + bias[channel] (+ residual)) on a dense (B,C,H,W) tensor in NCHW or channels-last
    memory (the residual must share y's memory format)."""
    B, Cc, H, W = _meta(y, "y", torch.float32, ANY4, "(B,C,H,W)").shape
    fmt = torch.contiguous_format if y.is_contiguous() else torch.channels_last
    if not y.is_contiguous(memory_format=fmt):
        raise _lib.IsxError("y must be dense NCHW or channels-last, has strides %s for shape %s" % (y.stride(), tuple(y.shape)))
    bias, rp = _f32(bias, "bias", Cc), _residual(residual, y.shape, fmt)
    _cuda(y=y, bias=bias, residual=residual)
    _launch("isx_bias_act_inplace", y.data_ptr(), bias.data_ptr(), rp, y.numel(), Cc, H * W if fmt is torch.contiguous_format else 1, 1 if relu else 0)
    return y


def images_u8_to_f32(img_u8, mean, std, channels_last=True):
    """ToTensor + Normalize on the GPU: (B,H,W,3) uint8 RGB -> (B,3,H,W) fp32 (channels-last memory by default)."""
    B, H, W, _ = _out(img_u8, (None, None, None, 3), torch.uint8, "img_u8").shape
    dev = _cuda(img_u8=img_u8)
    out = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    m, s_ = [float(v) for v in mean], [float(v) for v in std]
    _launch("isx_images_u8_to_f32", img_u8.data_ptr(), B, H, W, m[0], m[1], m[2], s_[0], s_[1], s_[2], 1 if channels_last else 0, out.data_ptr())
    return out


AFFINE_WORKSPACE_BUDGET = 1 << 30      # bytes of fp64 spline coefficients per launch of affine_noisy (24 bytes per pixel); larger batches go in chunks
_MEAN_STD = {}


def _mean_std_device(mean, std, device):
    """(6,) fp32 device tensor mean | std, cached per (values, device) for the life of the process (a constant is never dropped: a launch on
    some stream may still be reading it): the kernel reads them from device memory.  The constant is copied
    asynchronously from a pinned block on the stream that is current when it is first asked for (the host does not wait); a caller under ANOTHER
    stream is ordered behind that copy with an event wait until the copy has completed."""
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), device)
    entry = _MEAN_STD.get(key)
    stream = torch.cuda.current_stream(device)
    if entry is None:
        if len(key[0]) != 3 or len(key[1]) != 3 or 0.0 in key[1]:
            raise _lib.IsxError("mean and std must be three values each, std non-zero")
        t = torch.tensor(key[0] + key[1], dtype=torch.float32).pin_memory().to(device, non_blocking=True)
        created = torch.cuda.Event()
        created.record(stream)
        entry = _MEAN_STD[key] = [t, created, stream.cuda_stream]
    elif entry[1] is not None:
        if entry[1].query():
            entry[1] = None                     # visible to every stream from now on
        elif entry[2] != stream.cuda_stream:
            stream.wait_event(entry[1])
    return entry[0]


def affine_noisy(img_u8, rows, mats, seed, noise_ids, mean, std, channels_last=True, want_u8=False):
    """The reference's random_affine_noisy_cv + ToTensor + Normalize for a batch (isx_affine_noisy_u8): image b is row rows[b] of the
    (N,H,W,3) uint8 set `img_u8` (rows None: rows 0 .. B-1), warped by mats[b] = (m00, m01, t0, m10, m11, t1) (fp64), outside pixels filled with
    the noise of (seed, noise_ids[b]).  Returns the normalised (B,3,H,W) fp32 batch (channels-last memory by default), or (that, the warped
    (B,H,W,3) uint8 images) with want_u8.  mats / noise_ids / rows may be host arrays; they are copied to the device."""
    N, H, W, _ = _out(img_u8, (None, None, None, 3), torch.uint8, "img_u8").shape
    mats = torch.as_tensor(mats, dtype=torch.float64).reshape(-1, 6)
    B = mats.shape[0]
    noise_ids = torch.as_tensor(noise_ids, dtype=torch.int64).reshape(-1)
    if rows is not None:
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
    if noise_ids.numel() != B or (rows is not None and rows.numel() != B) or (rows is None and B > N):
        raise _lib.IsxError("affine_noisy: %d matrices, %d noise ids, %s rows, %d images" % (B, noise_ids.numel(), "no" if rows is None else rows.numel(), N))
    dev = _cuda(img_u8=img_u8)
    if not (mats.is_cuda or noise_ids.is_cuda or (rows is not None and rows.is_cuda)):
        # host parameters: ONE pinned block and one asynchronous copy for the three arrays (three pageable copies would each block the host)
        parts = [mats.contiguous().view(torch.int64).reshape(-1), noise_ids] + ([rows] if rows is not None else [])
        packed = torch.cat(parts).pin_memory().to(dev, non_blocking=True)
        mats, noise_ids = packed[:6 * B].view(torch.float64).view(B, 6), packed[6 * B:6 * B + noise_ids.numel()]
        rows = packed[6 * B + noise_ids.numel():] if rows is not None else None
    else:
        mats, noise_ids = mats.to(dev).contiguous(), noise_ids.to(dev).contiguous()
        rows = rows.to(dev).contiguous() if rows is not None else None
    ms = _mean_std_device(mean, std, dev)
    out = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    u8 = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8) if want_u8 else None
    if B == 0:
        return (out, u8) if want_u8 else out
    L = lib()
    per_image = int(L.isx_affine_noisy_workspace(1, H, W))
    if per_image == 0:
        raise _lib.IsxError("affine_noisy: images of %d x %d are refused (isx_affine_noisy_workspace)" % (H, W))
    chunk = int(max(1, min(B, 65535, AFFINE_WORKSPACE_BUDGET // per_image)))
    ws_bytes = int(L.isx_affine_noisy_workspace(chunk, H, W))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out_flat = out.permute(0, 2, 3, 1) if channels_last else out                       # a view whose dim 0 slices are contiguous memory
    seed = int(seed) & (2 ** 64 - 1)
    for s in range(0, B, chunk):
        n = min(chunk, B - s)
        _launch("isx_affine_noisy_u8", img_u8.data_ptr() if rows is not None else img_u8[s:].data_ptr(), None if rows is None else rows[s:].data_ptr(),
                n, H, W, mats[s:].data_ptr(), seed, noise_ids[s:].data_ptr(), ms.data_ptr(), ms[3:].data_ptr(), 1 if channels_last else 0,
                None if u8 is None else u8[s:].data_ptr(), out_flat[s:].data_ptr(), ws.data_ptr(), ws_bytes)
    return (out, u8) if want_u8 else out


# Optional per-launch timing of the trunk kernels (bench.py): a list that receives
# (kernel, algorithmic FLOP, algorithmic bytes, start event, end event) per call; None = off.
KERNEL_TIMER = None


def _timed(name, flop, nbytes, fn):
    if KERNEL_TIMER is None:
        return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    KERNEL_TIMER.append((name, flop, nbytes, a, b))
    return out


def _new_nhwc(shape, dev):
    return torch.empty(shape, device=dev, dtype=torch.float32, memory_format=torch.channels_last)


def bias_relu_maxpool(y, bias):
    """relu(y + bias[c]) -> MaxPool2d(3, 2, 1) of a channels-last (B,C,H,W) fp32 tensor in one pass."""
    B, Cc, H, W = _nhwc(y, "y")
    bias = _f32(bias, "bias", Cc)
    out = _new_nhwc((B, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), _cuda(y=y, bias=bias))
    _launch("isx_bias_relu_maxpool_nhwc", y.data_ptr(), bias.data_ptr(), B, H, W, Cc, out.data_ptr())
    return out


STEM_MAX_W = 896      # csrc/stem.hip: up to four column bands of 224 input columns


def stem7x7_pool_applicable(x, conv):
    """Can `stem7x7_pool` run this convolution (the ResNet stem: 3 -> 64, 7x7, stride 2, padding 3) on x?"""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[3] % 4 == 0 and x.shape[3] <= STEM_MAX_W
            and x.is_contiguous(memory_format=torch.channels_last) and conv.in_channels == 3 and conv.out_channels == 64
            and tuple(conv.kernel_size) == (7, 7) and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and x.data_ptr() % 16 == 0)


def stem7x7_pool(x, w_ohwi, bias):
    """relu(conv7x7 / stride 2 / padding 3 (x) + bias) -> MaxPool2d(3, 2, 1) of a channels-last (B,3,H,W) fp32 batch as ONE kernel.
    w_ohwi: (64,7,7,3) contiguous (= conv.weight.permute(0,2,3,1)).  Returns channels-last (B,64,Hp,Wp)."""
    B, _, H, W = _nhwc(x, "x", (None, 3, None, None), "(B,3,H,W)")
    w, bias = _f32(w_ohwi, "w_ohwi", (64, 7, 7, 3)), _f32(bias, "bias", 64)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = _new_nhwc((B, 64, Hp, Wp), _cuda(x=x, w_ohwi=w, bias=bias))
    _timed("isx_stem7x7_pool_nhwc", 2.0 * B * Hc * Wc * 147 * 64, 4.0 * (B * H * W * 3 + B * Hp * Wp * 64 + 147 * 64),
           lambda: _launch("isx_stem7x7_pool_nhwc", x.data_ptr(), B, H, W, w.data_ptr(), bias.data_ptr(), out.data_ptr()))
    return out


def conv1x1_nhwc(x, weight, bias, residual=None, relu=True):
    """1x1 stride-1 convolution of a channels-last (B,Cin,H,W) fp32 tensor with the epilogue fused:
    act(conv(x, weight) + bias (+ residual)) as ONE fp32-MFMA GEMM over the B*H*W pixels.  weight: (Cout,Cin[,1,1]).
    Returns a channels-last (B,Cout,H,W) tensor."""
    B, Cin, H, W = _nhwc(x, "x")
    w = _f32(_meta(weight, "weight").reshape(weight.shape[0], -1), "weight", (None, Cin), "(Cout, Cin)")
    Cout = w.shape[0]
    bias, rp = _f32(bias, "bias", Cout), _residual(residual, (B, Cout, H, W))
    y = _new_nhwc((B, Cout, H, W), _cuda(x=x, weight=w, bias=bias, residual=residual))
    px = B * H * W
    _timed("isx_conv1x1_nhwc", 2.0 * px * Cin * Cout, 4.0 * (px * Cin + px * Cout * (2 if rp else 1) + Cin * Cout),
           lambda: _launch("isx_conv1x1_nhwc", x.data_ptr(), px, Cin, w.data_ptr(), Cout, bias.data_ptr(), rp, 1 if relu else 0, y.data_ptr()))
    return y


def conv1x1_dual_nhwc(t, x, w_cat, bias, stride=1, relu=True):
    """act(conv1x1(t, w_cat[:, :K1]) + conv1x1(x[:, :, ::stride, ::stride], w_cat[:, K1:]) + bias) in one GEMM: the last
    convolution of a bottleneck block fused with its projection shortcut.  t: (B,K1,Ho,Wo), x: (B,K2,H,W), both channels-last."""
    B, K2, H, W = _nhwc(x, "x")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    K1 = _nhwc(t, "t", (B, None, Ho, Wo), "(B, K1, Ho, Wo) for x's shape and the stride")[1]
    w = _f32(w_cat, "w_cat", (None, K1 + K2), "(Cout, K1 + K2)")
    Cout = w.shape[0]
    bias = _f32(bias, "bias", Cout)
    y = _new_nhwc((B, Cout, Ho, Wo), _cuda(t=t, x=x, w_cat=w, bias=bias))
    px = B * Ho * Wo
    _timed("isx_conv1x1_dual_nhwc", 2.0 * px * (K1 + K2) * Cout, 4.0 * (px * (K1 + K2) + px * Cout + (K1 + K2) * Cout),
           lambda: _launch("isx_conv1x1_dual_nhwc", t.data_ptr(), K1, x.data_ptr(), B, H, W, K2, stride, w.data_ptr(), Cout, bias.data_ptr(),
                           1 if relu else 0, y.data_ptr()))
    return y


def conv3x3_nhwc(x, w_ohwi, bias, stride=1, residual=None, relu=True):
    """3x3 convolution (padding 1, stride 1|2) of a channels-last (B,Cin,H,W) fp32 tensor, epilogue fused.
    w_ohwi: (Cout,3,3,Cin) contiguous (= conv.weight.permute(0,2,3,1)).  Returns channels-last (B,Cout,Ho,Wo)."""
    B, Cin, H, W = _nhwc(x, "x")
    w = _f32(w_ohwi, "w_ohwi", (None, 3, 3, Cin), "(Cout, 3, 3, Cin)")
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bias, rp = _f32(bias, "bias", Cout), _residual(residual, (B, Cout, Ho, Wo))
    y = _new_nhwc((B, Cout, Ho, Wo), _cuda(x=x, w_ohwi=w, bias=bias, residual=residual))
    _timed("isx_conv3x3_nhwc", 18.0 * B * Ho * Wo * Cin * Cout, 4.0 * (B * H * W * Cin + B * Ho * Wo * Cout * (2 if rp else 1) + 9 * Cin * Cout),
           lambda: _launch("isx_conv3x3_nhwc", x.data_ptr(), B, H, W, Cin, w.data_ptr(), Cout, stride, bias.data_ptr(), rp, 1 if relu else 0,
                           y.data_ptr()))
    return y


def conv3x3_expand_nhwc(x, w2_ohwi, b2, stride, w3t, b3, residual=None, relu=True):
    """conv2 + conv3 of a Bottleneck with 64 mid channels as ONE kernel: act(W3 . relu(conv3x3(x, W2) + b2) + b3 (+ residual)).
    x: channels-last (B,Cin,H,W); w2_ohwi: (64,3,3,Cin); w3t: (64,256) = conv3.weight.view(256,64).t().contiguous().
    Returns channels-last (B,256,Ho,Wo)."""
    B, Cin, H, W = _nhwc(x, "x")
    w2, w3 = _f32(w2_ohwi, "w2_ohwi", (64, 3, 3, Cin), "(64, 3, 3, Cin)"), _f32(w3t, "w3t", (64, None), "(64, Cout)")
    Cout = w3.shape[1]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    b2, b3, rp = _f32(b2, "b2", 64), _f32(b3, "b3", Cout), _residual(residual, (B, Cout, Ho, Wo))
    y = _new_nhwc((B, Cout, Ho, Wo), _cuda(x=x, w2_ohwi=w2, w3t=w3, b2=b2, b3=b3, residual=residual))
    _timed("isx_conv3x3_expand_nhwc", 2.0 * B * Ho * Wo * (9 * Cin * 64 + 64 * Cout),
           4.0 * (B * H * W * Cin + B * Ho * Wo * Cout * (2 if rp else 1) + 9 * Cin * 64 + 64 * Cout),
           lambda: _launch("isx_conv3x3_expand_nhwc", x.data_ptr(), B, H, W, Cin, w2.data_ptr(), b2.data_ptr(), stride, w3.data_ptr(), Cout,
                           b3.data_ptr(), rp, 1 if relu else 0, y.data_ptr()))
    return y


def conv3x3_expand128_nhwc(x, w2_ohwi, b2, w3t, b3, residual=None, relu=True):
    """conv2 + conv3 of an identity Bottleneck with 128 mid channels as ONE kernel: act(W3 . relu(conv3x3(x, W2) + b2) + b3 (+ residual)), stride 1.
    x: channels-last (B,Cin,H,W), Cin % 64 == 0; w2_ohwi: (128,3,3,Cin); w3t: (128,Cout) = conv3.weight.view(Cout,128).t().contiguous(),
    Cout % 128 == 0.  Returns channels-last (B,Cout,H,W)."""
    B, Cin, H, W = _nhwc(x, "x")
    w2, w3 = _f32(w2_ohwi, "w2_ohwi", (128, 3, 3, Cin), "(128, 3, 3, Cin)"), _f32(w3t, "w3t", (128, None), "(128, Cout)")
    Cout = w3.shape[1]
    if Cin % 64 != 0 or Cout % 128 != 0:
        raise _lib.IsxError("Cin must be a multiple of 64 and Cout a multiple of 128")
    b2, b3, rp = _f32(b2, "b2", 128), _f32(b3, "b3", Cout), _residual(residual, (B, Cout, H, W))
    y = _new_nhwc((B, Cout, H, W), _cuda(x=x, w2_ohwi=w2, w3t=w3, b2=b2, b3=b3, residual=residual))
    px = B * H * W
    _timed("isx_conv3x3_expand128_nhwc", 2.0 * px * (9 * Cin * 128 + 128 * Cout),
           4.0 * (px * Cin + px * Cout * (2 if rp else 1) + 9 * Cin * 128 + 128 * Cout),
           lambda: _launch("isx_conv3x3_expand128_nhwc", x.data_ptr(), B, H, W, Cin, w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), Cout, b3.data_ptr(),
                           rp, 1 if relu else 0, y.data_ptr()))
    return y


def conv3x3_expand_dual_nhwc(t, w2_ohwi, b2, x2, wcat_t, bias, relu=True):
    """First block of a 64-mid-channel stage as ONE kernel: act([W3 | Wd] . [relu(conv3x3(t, W2) + b2) ; x2] + bias), stride 1.
    t: channels-last (B,Cin,H,W); x2: channels-last (B,64,H,W); wcat_t: (128,256) = cat([W3, Wd], 1).t().contiguous()."""
    B, Cin, H, W = _nhwc(t, "t")
    _nhwc(x2, "x2", (B, 64, H, W), "(B, 64, H, W)")
    w2, wc = _f32(w2_ohwi, "w2_ohwi", (64, 3, 3, Cin), "(64, 3, 3, Cin)"), _f32(wcat_t, "wcat_t", (128, None), "(128, Cout)")
    Cout = wc.shape[1]
    b2, bias = _f32(b2, "b2", 64), _f32(bias, "bias", Cout)
    y = _new_nhwc((B, Cout, H, W), _cuda(t=t, x2=x2, w2_ohwi=w2, wcat_t=wc, b2=b2, bias=bias))
    _timed("isx_conv3x3_expand_nhwc", 2.0 * B * H * W * (9 * Cin * 64 + 128 * Cout),
           4.0 * (B * H * W * (Cin + 64 + Cout) + 9 * Cin * 64 + 128 * Cout),
           lambda: _launch("isx_conv3x3_expand_dual_nhwc", t.data_ptr(), B, H, W, Cin, w2.data_ptr(), b2.data_ptr(), x2.data_ptr(), wc.data_ptr(), Cout,
                           bias.data_ptr(), 1 if relu else 0, y.data_ptr()))
    return y


def boxpool_s1(fmap, kh, kw):
    fmap = _f32(fmap, "fmap", ANY4, "(B,C,H,W)")
    B, Cc, H, W = fmap.shape
    out = torch.empty((B, Cc, H - kh + 1, W - kw + 1), device=_cuda(fmap=fmap), dtype=torch.float32)
    _launch("isx_boxpool_s1", fmap.data_ptr(), B, Cc, H, W, kh, kw, out.data_ptr())
    return out


def _is_nhwc(t):
    """A 4-d tensor whose MEMORY is channels-last and not also plain contiguous (sizes where both hold are treated as NCHW)."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def boxpool_s1_applicable_nhwc(fmap):
    return (fmap.is_cuda and fmap.dtype == torch.float32 and _is_nhwc(fmap) and fmap.shape[1] % 4 == 0
            and fmap.shape[2] * fmap.shape[3] * 16 <= 64 * 1024 and fmap.data_ptr() % 16 == 0)


def boxpool_s1_nhwc(fmap, kh, kw):
    """AvgPool2d((kh,kw), stride 1) of a channels-last (B,C,H,W) map, result channels-last: no transpose on the way in or out."""
    B, Cc, H, W = _nhwc(fmap, "fmap")
    if Cc % 4 != 0 or H * W > 4096 or fmap.data_ptr() % 16 != 0:
        raise _lib.IsxError("fmap %s must have C %% 4 == 0 and H*W <= 4096 and start on a 16-byte boundary" % (tuple(fmap.shape),))
    out = _new_nhwc((B, Cc, H - kh + 1, W - kw + 1), _cuda(fmap=fmap))
    _launch("isx_boxpool_s1_nhwc", fmap.data_ptr(), B, Cc, H, W, kh, kw, out.data_ptr())
    return out


def best_location_desc(cls, eps=EPS):
    """cls (B,K,Hp,Wp) class-score maps -> (desc (B,K), loc (B,2)); a channels-last tensor is consumed in place."""
    B, K, Hp, Wp = _meta(cls, "cls", torch.float32, ANY4, "(B,K,Hp,Wp)").shape
    dev = _cuda(cls=cls)
    desc = torch.empty((B, K), device=dev, dtype=torch.float32)
    loc = torch.empty((B, 2), device=dev, dtype=torch.int64)
    if _is_nhwc(cls):
        _launch("isx_best_location_desc_nhwc", cls.data_ptr(), B, K, Hp, Wp, eps, desc.data_ptr(), loc.data_ptr())
        return desc, loc
    cls = cls.contiguous()
    _launch("isx_best_location_desc", cls.data_ptr(), B, K, Hp, Wp, eps, desc.data_ptr(), loc.data_ptr())
    return desc, loc


def region_topk(cls, k):
    """Canonical top-k locations of the class-max map.  cls (K,Hp,Wp) -> (idx (k), score (k));
    cls (B,K,Hp,Wp) -> (idx (B,k), score (B,k))."""
    single = _meta(cls, "cls", torch.float32).dim() == 3
    if single:
        cls = cls.unsqueeze(0)
    B, K, Hp, Wp = _meta(cls, "cls", None, ANY4, "(K,Hp,Wp) or (B,K,Hp,Wp)").shape
    sc, idx = _topk_out(B, k, cls=cls)
    if _is_nhwc(cls):                  # channels-last score map (1x1-convolution classifier on the NHWC trunk): consumed in place
        _launch("isx_region_topk_nhwc", cls.data_ptr(), B, K, Hp, Wp, k, idx.data_ptr(), sc.data_ptr())
    else:
        cls = cls.contiguous()
        _launch("isx_region_topk", cls.data_ptr(), B, K, Hp, Wp, k, idx.data_ptr(), sc.data_ptr())
    return (idx[0], sc[0]) if single else (idx, sc)


def _region_args(fmap, flat_idx, taps, shift=None, name="shift"):
    """The arguments the NHWC region entries share: channels-last fmap with C % 4 == 0, flat_idx (B, k >= 1), the Shift (C * taps) or None."""
    B, Cc, Hf, Wf = _nhwc(fmap, "fmap", what="(B,C,Hf,Wf)")
    flat_idx = _typed(flat_idx, torch.int64, "flat_idx", (B, None))
    if Cc % 4 != 0 or flat_idx.size(1) < 1:
        raise _lib.IsxError("fmap %s needs C %% 4 == 0 and flat_idx %s k >= 1" % (tuple(fmap.shape), tuple(flat_idx.shape)))
    return flat_idx, shift if shift is None else _f32(shift, name, Cc * taps, "C*kh*kw")


def region_gather_l2_nhwc(fmap, kh, kw, flat_idx, Wp, shift_hwc=None, eps=EPS):
    """Window gather + L2 + Shift on a channels-last (B,C,Hf,Wf) map; rows (B,k,kh*kw*C) keep the window in (h,w,C) order
    (row[(a*kw + b)*C + c]); shift_hwc: the Shift parameter in that order."""
    flat_idx, shift_hwc = _region_args(fmap, flat_idx, kh * kw, shift_hwc, "shift_hwc")
    B, Cc, Hf, Wf = fmap.shape
    k = flat_idx.size(1)
    rows = torch.empty((B, k, Cc * kh * kw), device=_cuda(fmap=fmap, flat_idx=flat_idx, shift_hwc=shift_hwc), dtype=torch.float32)
    _launch("isx_region_gather_l2_nhwc", fmap.data_ptr(), B, Cc, Hf, Wf, kh, kw, flat_idx.data_ptr(), k, Wp, _ptr(shift_hwc), eps, rows.data_ptr())
    return rows


def region_sum_l2_nhwc(fmap, kh, kw, flat_idx, Wp, shift=None, eps=EPS):
    """The k windows of every image gathered, L2-normalised, shifted and summed in window order (isx_region_sum_l2_nhwc): fmap channels-last
    (B,C,Hf,Wf), flat_idx (B,k) -> (rows (B, C*kh*kw) in (c, a, b) order -- the Linear's stored column order, `shift` in that order too --,
    n2 (B,k) for region_sum_l2_bwd_nhwc).  An index outside the map is skipped."""
    flat_idx, shift = _region_args(fmap, flat_idx, kh * kw, shift)
    B, Cc, Hf, Wf = fmap.shape
    k = flat_idx.size(1)
    dev = _cuda(fmap=fmap, flat_idx=flat_idx, shift=shift)
    rows = torch.empty((B, Cc * kh * kw), device=dev, dtype=torch.float32)
    n2 = torch.empty((B, k), device=dev, dtype=torch.float32)
    _launch("isx_region_sum_l2_nhwc", fmap.data_ptr(), B, Cc, Hf, Wf, kh, kw, flat_idx.data_ptr(), k, Wp, _ptr(shift), eps, rows.data_ptr(), n2.data_ptr())
    return rows, n2


def region_sum_l2_bwd_nhwc(fmap, g, n2, kh, kw, flat_idx, Wp, add=None, add_every=1):
    """Backward of region_sum_l2_nhwc (isx_region_sum_l2_bwd_nhwc): g (B, C*kh*kw) the gradient wrt the rows, n2 (B,k) as the forward wrote
    it, add (channels-last (B / add_every, C, Hf, Wf)) or None: a further gradient of the map for every add_every-th image (0, add_every,
    ...), added last.  Returns the channels-last (B,C,Hf,Wf) gradient."""
    flat_idx, _ = _region_args(fmap, flat_idx, kh * kw)
    B, Cc, Hf, Wf = fmap.shape
    k = flat_idx.size(1)
    g, n2 = _f32(g, "g", (B, Cc * kh * kw), "(B, C*kh*kw)"), _f32(n2, "n2", (B, k), "(B, k)")
    if add is not None:
        if add_every < 1 or B % add_every:
            raise _lib.IsxError("region_sum_l2_bwd_nhwc: %d images do not split into groups of %d" % (B, add_every))
        _nhwc(add, "add", (B // add_every, Cc, Hf, Wf), "(B / add_every, C, Hf, Wf)")
    dev = _cuda(fmap=fmap, flat_idx=flat_idx, g=g, n2=n2, add=add)
    cw = torch.empty((B, k), device=dev, dtype=torch.float32)
    dx = torch.empty((B, Hf, Wf, Cc), device=dev, dtype=torch.float32)
    _launch("isx_region_sum_l2_bwd_nhwc", fmap.data_ptr(), g.data_ptr(), n2.data_ptr(), B, Cc, Hf, Wf, kh, kw, flat_idx.data_ptr(), k, Wp, _ptr(add),
            add_every if add is not None else 1, cw.data_ptr(), dx.data_ptr())
    return dx.permute(0, 3, 1, 2)


def region_gather_l2(fmap, kh, kw, flat_idx, Wp, shift=None, eps=EPS):
    """Window gather + L2 + Shift.  fmap (C,Hf,Wf), flat_idx (k) -> rows (k,F); batched: fmap (B,C,Hf,Wf),
    flat_idx (B,k) -> rows (B,k,F)."""
    single = _meta(fmap, "fmap").dim() == 3
    if single:
        fmap, flat_idx = fmap.unsqueeze(0), _meta(flat_idx, "flat_idx").reshape(1, -1)
    fmap = _f32(fmap, "fmap", ANY4, "(C,Hf,Wf) or (B,C,Hf,Wf)")
    B, Cc, Hf, Wf = fmap.shape
    flat_idx = _typed(flat_idx, torch.int64, "flat_idx", (B, None))
    k = flat_idx.size(1)
    shift = shift if shift is None else _f32(shift, "shift", Cc * kh * kw, "C*kh*kw")
    rows = torch.empty((B, k, Cc * kh * kw), device=_cuda(fmap=fmap, flat_idx=flat_idx, shift=shift), dtype=torch.float32)
    _launch("isx_region_gather_l2", fmap.data_ptr(), B, Cc, Hf, Wf, kh, kw, flat_idx.data_ptr(), k, Wp, _ptr(shift), eps, rows.data_ptr())
    return rows[0] if single else rows


def _pair(Q, G, dtype=torch.float32, names=("Q", "G")):
    """Query rows (M, D) against gallery rows (N, D): (Q, G, M, N, D), both contiguous."""
    Q = _meta(Q, names[0], dtype, (None, None), "(M, D)").contiguous()
    G = _meta(G, names[1], dtype, (None, Q.shape[1]), "(N, D)").contiguous()
    return Q, G, Q.shape[0], G.shape[0], Q.shape[1]


def _sim_out(out, M, N, **inputs):
    """An (M, N) float32 result matrix: the caller's `out`, checked, or a new one, after the device check of the inputs."""
    if out is None:
        return torch.empty((M, N), device=_cuda(**inputs), dtype=torch.float32)
    _cuda(**inputs, out=_out(out, (M, N), torch.float32, "out"))
    return out


def cosine_sim(Q, G, out=None):
    Q, G, M, N, D = _pair(Q, G)
    sim = _sim_out(out, M, N, Q=Q, G=G)
    _launch("isx_cosine_sim", Q.data_ptr(), M, G.data_ptr(), N, D, sim.data_ptr())
    return sim


def cosine_topk_workspace(M, N, D, k):
    return lib().isx_cosine_topk_workspace(M, N, D, k)


def cosine_topk(Q, G, k, idx_base=0, ws=None, out=None):
    """(top_score (M,k) f32, top_idx (M,k) i64), canonical order.  `ws`: optional uint8 CUDA
    tensor reused across calls (sized by cosine_topk_workspace or larger/smaller)."""
    Q, G, M, N, D = _pair(Q, G)
    ws = ws if ws is None else _out(ws, (None,), torch.uint8, "ws")
    ts, ti = _topk_out(M, k, out, Q=Q, G=G, ws=ws)
    if ws is None:
        ws = torch.empty((cosine_topk_workspace(M, N, D, k),), device=Q.device, dtype=torch.uint8)
    _launch("isx_cosine_topk", Q.data_ptr(), M, G.data_ptr(), N, D, k, idx_base, ts.data_ptr(), ti.data_ptr(), ws.data_ptr(), ws.numel())
    return ts, ti


def gallery_to_f16(G):
    """(Gh (N,D) fp16 scaled image, gstats (4,) f32: max |g|^2, max |G|, max conversion loss^2, 0) -- the cached gallery side of cosine_topk_fast."""
    G = _f32(G, "G", (None, None))
    N, D = G.shape
    dev = _cuda(G=G)
    Gh = torch.empty((N, D), device=dev, dtype=torch.float16)
    gstats = torch.empty((4,), device=dev, dtype=torch.float32)
    _launch("isx_gallery_to_f16", G.data_ptr(), N, D, Gh.data_ptr(), gstats.data_ptr())
    return Gh, gstats


def cosine_topk_fast_workspace(M, N, D, k, have_gallery_f16=False):
    return lib().isx_cosine_topk_fast_workspace(M, N, D, k, 1 if have_gallery_f16 else 0)


def cosine_topk_fast_fallback_counter(ws, M, N, D, k, have_gallery_f16=False):
    """int32 view (1 element, on the device) of the fallback-row counter inside a cosine_topk_fast workspace, or None when a
    call of this shape runs the fp32 search as a whole.  Valid once the search has completed on its stream."""
    off = lib().isx_cosine_topk_fast_fallback_offset(M, N, D, k, 1 if have_gallery_f16 else 0)
    if off == (1 << 64) - 1 or off + 4 > ws.numel():
        return None
    return ws[off:off + 4].view(torch.int32)


def cosine_topk_fast(Q, G, k, idx_base=0, gallery_f16=None, ws=None, out=None):
    """Same result as cosine_topk, bit for bit; fp16-MFMA filter + exact fp32 re-scoring.
    gallery_f16: optional (Gh, gstats) from gallery_to_f16(G)."""
    Q, G, M, N, D = _pair(Q, G)
    Gh = gstats = None
    if gallery_f16 is not None:
        Gh, gstats = _out(gallery_f16[0], (N, D), torch.float16, "gallery_f16[0]"), _out(gallery_f16[1], 4, torch.float32, "gallery_f16[1]")
    ws = ws if ws is None else _out(ws, (None,), torch.uint8, "ws")
    ts, ti = _topk_out(M, k, out, Q=Q, G=G, ws=ws, **{"gallery_f16[0]": Gh, "gallery_f16[1]": gstats})
    if ws is None:
        ws = torch.empty((cosine_topk_fast_workspace(M, N, D, k, gallery_f16 is not None),), device=Q.device, dtype=torch.uint8)
    _launch("isx_cosine_topk_fast", Q.data_ptr(), M, G.data_ptr(), N, D, k, idx_base, _ptr(Gh), _ptr(gstats), ts.data_ptr(), ti.data_ptr(),
            ws.data_ptr(), ws.numel())
    return ts, ti


def _row_segments(M, N, k):
    """Segments per row for a FEW-ROW top-k (0 = one launch over whole rows).  `isx_topk_rows` gives every row one workgroup: with fewer rows
    than the chip holds workgroups (1 000 queries x 100 000 gallery rows: 0.43 ms, 0.9 TB/s) the launch is latency-bound.  A row-major
    (M, N) matrix IS an (M S, N / S) matrix when S divides N, so the same kernel selects per segment and `isx_topk_merge` (canonical
    comparator on the restored column indices) merges the S lists of a row: same result, bit for bit."""
    if M >= 4096 or N < 16384 or k > 256:
        return 0
    target = max(2, 8192 // max(M, 1))               # one wave per segment: ~8 waves per SIMD fill the chip; more only adds merge work
    best = 0
    for S in range(2, min(64, 4096 // max(k, 1)) + 1):
        if N % S == 0 and N // S >= max(k, 1024) and (best == 0 or abs(S - target) < abs(best - target)):
            best = S
    return best


def topk_rows(sim, k, idx_base=0):
    sim = _f32(sim, "sim", (None, None))
    M, N = sim.shape
    S = _row_segments(M, N, k)
    if S:
        L = N // S
        ts, ti = _topk_out(M * S, k, sim=sim)
        _launch("isx_topk_rows", sim.data_ptr(), M * S, L, k, 0, ts.data_ptr(), ti.data_ptr())
        ti = ti.view(M, S, k) + (torch.arange(S, device=sim.device, dtype=torch.int64) * L + idx_base).view(1, S, 1)
        return topk_merge(ts.view(M, S, k).permute(1, 0, 2).contiguous(), ti.permute(1, 0, 2).contiguous())
    ts, ti = _topk_out(M, k, sim=sim)
    _launch("isx_topk_rows", sim.data_ptr(), M, N, k, idx_base, ts.data_ptr(), ti.data_ptr())
    return ts, ti


def rank_full(sim):
    sim = _f32(sim, "sim", (None, None))
    M, N = sim.shape
    ranked = torch.empty((M, N), device=_cuda(sim=sim), dtype=torch.int64)
    nb = lib().isx_rank_full_workspace(M, N)
    ws = torch.empty((nb,), device=sim.device, dtype=torch.uint8)
    _launch("isx_rank_full", sim.data_ptr(), M, N, ranked.data_ptr(), ws.data_ptr(), nb)
    return ranked


def _labels(M, N, qlab, glab):
    """int32 labels of the M query rows and the N gallery rows of a score (or rank) matrix."""
    return _typed(qlab, torch.int32, "qlab", M), _typed(glab, torch.int32, "glab", N)


def average_precision(ranked, qlab, glab, kth=1):
    ranked = _typed(ranked, torch.int64, "ranked", (None, None))
    M, N = ranked.shape
    qlab, glab = _labels(M, N, qlab, glab)
    ap = torch.empty((M,), device=_cuda(ranked=ranked, qlab=qlab, glab=glab), dtype=torch.float64)
    _launch("isx_average_precision", ranked.data_ptr(), M, N, qlab.data_ptr(), glab.data_ptr(), kth, ap.data_ptr())
    return ap


def average_precision_sim(sim, qlab, glab, kth=1):
    """AP per query straight from the score matrix (no sort).  Rows with more than 2048 positives are
    recomputed through rank_full + average_precision, so the result always equals the sorted path."""
    sim = _f32(sim, "sim", (None, None))
    M, N = sim.shape
    qlab, glab = _labels(M, N, qlab, glab)
    ap = torch.empty((M,), device=_cuda(sim=sim, qlab=qlab, glab=glab), dtype=torch.float64)
    _launch("isx_average_precision_sim", sim.data_ptr(), M, N, qlab.data_ptr(), glab.data_ptr(), kth, ap.data_ptr())
    heavy = (ap == -1.0).nonzero().flatten()
    if heavy.numel():
        ap[heavy] = average_precision(rank_full(sim[heavy]), qlab[heavy], glab, kth)
    return ap


def ap_shard_max_positives():
    return int(lib().isx_ap_shard_max_positives())


def ap_shard_positives(sim, idx_base, qlab, glab, cap=None):
    """Step 1 of the sharded average precision (include/isx.h): (keys (M, cap) int64 bit patterns of the canonical uint64 keys, 0 = empty;
    count (M,) int32) of this shard's positives per query.  sim: (M, Ns) scores against the shard's rows, idx_base: the shard's first global row."""
    sim = _f32(sim, "sim", (None, None))
    M, N = sim.shape
    qlab, glab = _labels(M, N, qlab, glab)
    dev = _cuda(sim=sim, qlab=qlab, glab=glab)
    cap = ap_shard_max_positives() if cap is None else int(cap)
    keys = torch.empty((M, cap), dtype=torch.int64, device=dev)
    count = torch.empty((M,), dtype=torch.int32, device=dev)
    _launch("isx_ap_shard_positives", sim.data_ptr(), M, N, int(idx_base), qlab.data_ptr(), glab.data_ptr(), cap, keys.data_ptr(), count.data_ptr())
    return keys, count


def ap_shard_hist(sim, idx_base, keys_all):
    """Step 2: this shard's bucket counts (M, ap_shard_max_positives()) int32 against the gathered keys of all shards (M, W)."""
    sim = _f32(sim, "sim", (None, None))
    M, N = sim.shape
    keys_all = _typed(keys_all, torch.int64, "keys_all", (M, None))
    dev = _cuda(sim=sim, keys_all=keys_all)
    hist = torch.empty((M, ap_shard_max_positives()), dtype=torch.int32, device=dev)
    _launch("isx_ap_shard_hist", sim.data_ptr(), M, N, int(idx_base), keys_all.data_ptr(), int(keys_all.size(1)), hist.data_ptr())
    return hist


def ap_from_hist(hist, n_lab, kth=1):
    """Step 3: float64 AP per query from the histogram summed over the shards (M, ld) and the positives per query over all shards (M,)."""
    hist = _typed(hist, torch.int32, "hist", (None, None))
    M = hist.size(0)
    n_lab = _typed(n_lab, torch.int32, "n_lab", M)
    ap = torch.empty((M,), dtype=torch.float64, device=_cuda(hist=hist, n_lab=n_lab))
    _launch("isx_ap_from_hist", hist.data_ptr(), int(hist.size(1)), n_lab.data_ptr(), M, int(kth), ap.data_ptr())
    return ap


def masked_sums(sim, qlab, glab):
    sim = _f32(sim, "sim", (None, None))
    M, N = sim.shape
    qlab, glab = _labels(M, N, qlab, glab)
    out = torch.empty((M, 2), device=_cuda(sim=sim, qlab=qlab, glab=glab), dtype=torch.float64)
    _launch("isx_masked_sums", sim.data_ptr(), M, N, qlab.data_ptr(), glab.data_ptr(), out.data_ptr())
    return out


def tree_sum_rows(rows, out=None):
    """Sum of the rows of a (L, n) fp32 device tensor in the canonical tree order of isx/dp.py (tree_sum), one kernel (isx_tree_sum_rows);
    L <= 16.  `out`: an (n,) tensor to write (may be rows[0])."""
    rows = _f32(rows, "rows", (None, None))
    L, n = rows.shape
    out = out if out is None else _out(out, (n,), torch.float32, "out")
    dev = _cuda(rows=rows, out=out)
    if out is None:
        out = torch.empty((n,), device=dev, dtype=torch.float32)
    _launch("isx_tree_sum_rows", rows.data_ptr(), int(L), int(rows.stride(0)) if L > 1 else int(n), int(n), out.data_ptr())
    return out


DBA_MAX_GROUP = 1024


def dba_groups(emb, order, grp_begin, grp_size, max_group, k=-1):
    """DBA (reference test/instance_avg.py:7-33) over same-instance groups of at most DBA_MAX_GROUP items; see include/isx.h."""
    emb = _f32(emb, "emb", (None, None))
    N, D = emb.shape
    order, grp_begin, grp_size = (_typed(t, torch.int32, n, N) for t, n in ((order, "order"), (grp_begin, "grp_begin"), (grp_size, "grp_size")))
    _cuda(emb=emb, order=order, grp_begin=grp_begin, grp_size=grp_size)
    out = torch.empty_like(emb)
    _launch("isx_dba_groups", emb.data_ptr(), N, D, order.data_ptr(), grp_begin.data_ptr(), grp_size.data_ptr(), int(max_group), int(k), out.data_ptr())
    return out


def topk_merge(scores, idx):
    scores = _f32(scores, "scores", (None, None, None), "(P, M, k)")
    idx = _typed(idx, torch.int64, "idx", tuple(scores.shape))
    P, M, k = scores.shape
    os_, oi = _topk_out(M, k, scores=scores, idx=idx)
    _launch("isx_topk_merge", scores.data_ptr(), idx.data_ptr(), P, M, k, os_.data_ptr(), oi.data_ptr())
    return os_, oi


# ---- native RCCL exchange of per-shard top-k lists (lazy-bound librccl; see csrc/comm.cpp) -------------
def comm_unique_id():
    """bytes of an ncclUniqueId (create on rank 0, ship to the other ranks by any means)."""
    import ctypes
    n = lib().isx_comm_unique_id_bytes()
    buf = ctypes.create_string_buffer(n)
    _call("isx_comm_unique_id", ctypes.cast(buf, ctypes.c_void_p))
    return bytes(buf.raw)


def comm_init_rank(nranks, rank, unique_id):
    """ncclComm_t handle (an int) of this rank; the current CUDA device must already be set."""
    import ctypes
    handle = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(unique_id, len(unique_id))
    _call("isx_comm_init_rank", ctypes.byref(handle), nranks, rank, ctypes.cast(buf, ctypes.c_void_p))
    return handle.value


def comm_destroy(comm):
    _call("isx_comm_destroy", comm)


def shard_topk_allgather(comm, nranks, s_local, i_local):
    """(P,M,k) scores and indices gathered from every rank (rank-major), on the current stream."""
    s_local = _f32(s_local, "s_local", (None, None), "(M, k)")
    i_local = _typed(i_local, torch.int64, "i_local", tuple(s_local.shape))
    M, k = s_local.shape
    dev = _cuda(s_local=s_local, i_local=i_local)
    all_s = torch.empty((nranks, M, k), device=dev, dtype=torch.float32)
    all_i = torch.empty((nranks, M, k), device=dev, dtype=torch.int64)
    _launch("isx_shard_topk_allgather", comm, s_local.data_ptr(), i_local.data_ptr(), M, k, all_s.data_ptr(), all_i.data_ptr())
    return all_s, all_i


def comm_allgather_rows(comm, nranks, rows_local, out=None):
    """(P * rows, D) descriptor rows of every rank (rank-major) on libisx's communicator, on the current stream."""
    rows_local = _f32(rows_local, "rows_local", (None, None))
    R, D = rows_local.shape
    out = _sim_out(out, nranks * R, D, rows_local=rows_local)
    _launch("isx_comm_allgather_rows", comm, rows_local.data_ptr(), R, D, out.data_ptr())
    return out


# ---- training step -----------------------------------------------------------------------
def mine_negatives(sim, labels, i1, i2, semi_hard, row_base=0):
    """neg index per positive couple (int64, -1 = none available).  sim: the N x N matrix, or rows
    [row_base, row_base + sim.size(0)) of it (every anchor i1 inside that range; i1 / i2 are absolute indices)."""
    sim = _f32(sim, "sim", (None, None))
    rows, N = sim.shape
    labels = _typed(labels, torch.int32, "labels", N)
    i1 = _typed(i1, torch.int64, "i1")
    i2 = _typed(i2, torch.int64, "i2", i1.numel())
    _cuda(sim=sim, labels=labels, i1=i1, i2=i2)
    neg = torch.empty_like(i1)
    if rows == N and row_base == 0:
        _launch("isx_mine_negatives", sim.data_ptr(), N, labels.data_ptr(), i1.data_ptr(), i2.data_ptr(), i1.numel(), 1 if semi_hard else 0, neg.data_ptr())
        return neg
    if i1.numel() and not (int(i1.min()) >= row_base and int(i1.max()) < row_base + rows):
        raise _lib.IsxError("mine_negatives: anchors outside the row block [%d, %d)" % (row_base, row_base + rows))
    _launch("isx_mine_negatives_rows", sim.data_ptr(), N, row_base, rows, labels.data_ptr(), i1.data_ptr(), i2.data_ptr(), i1.numel(),
            1 if semi_hard else 0, neg.data_ptr())
    return neg


def _triplet(anchor, pos, neg):
    """anchor, pos, neg: three float32 (B, D) blocks of one shape."""
    anchor = _f32(anchor, "anchor", (None, None), "(B, D)")
    return anchor, _f32(pos, "pos", tuple(anchor.shape), "anchor's shape"), _f32(neg, "neg", tuple(anchor.shape), "anchor's shape")


def triplet_loss_rows(anchor, pos, neg, margin, normalized=True):
    anchor, pos, neg = _triplet(anchor, pos, neg)
    B, D = anchor.shape
    rows = torch.empty((B,), device=_cuda(anchor=anchor, pos=pos, neg=neg), dtype=torch.float32)
    _launch("isx_triplet_loss_fwd", anchor.data_ptr(), pos.data_ptr(), neg.data_ptr(), B, D, margin, 1 if normalized else 0, rows.data_ptr())
    return rows


def triplet_loss_grads(anchor, pos, neg, loss_rows, scale, normalized=True, scale_dev=None):
    """scale_dev: optional 1-element float32 CUDA tensor (autograd's grad_output) multiplied in on the device -- no host synchronisation."""
    anchor, pos, neg = _triplet(anchor, pos, neg)
    B, D = anchor.shape
    loss_rows = _f32(loss_rows, "loss_rows", B)
    sd_ = scale_dev if scale_dev is None else _f32(_meta(scale_dev, "scale_dev").reshape(-1), "scale_dev", 1)
    _cuda(anchor=anchor, pos=pos, neg=neg, loss_rows=loss_rows, scale_dev=sd_)
    ga, gp, gn = torch.empty_like(anchor), torch.empty_like(anchor), torch.empty_like(anchor)
    if sd_ is not None:
        _launch("isx_triplet_loss_bwd_dev", anchor.data_ptr(), pos.data_ptr(), neg.data_ptr(), loss_rows.data_ptr(), B, D, float(scale), sd_.data_ptr(),
                1 if normalized else 0, ga.data_ptr(), gp.data_ptr(), gn.data_ptr())
        return ga, gp, gn
    _launch("isx_triplet_loss_bwd", anchor.data_ptr(), pos.data_ptr(), neg.data_ptr(), loss_rows.data_ptr(), B, D, float(scale),
            1 if normalized else 0, ga.data_ptr(), gp.data_ptr(), gn.data_ptr())
    return ga, gp, gn


def triplet_leaves(d_all, leaves, margin, normalized=True, scale_a=1.0, scale_b=1.0):
    """Triplet loss + gradient of every micro-batch of a step in one launch (isx_triplet_leaves).  d_all: (leaves * 3 k, D), per leaf the anchor,
    positive and negative rows.  Returns (per-leaf sum of the row losses (leaves,), gradient rows like d_all scaled by scale_a * scale_b)."""
    d_all = _f32(d_all, "d_all", (None, None))
    R, D = d_all.shape
    if leaves <= 0 or R % (3 * leaves):
        raise _lib.IsxError("triplet_leaves: %d rows do not split into %d leaves of 3 k rows" % (R, leaves))
    k = R // (3 * leaves)
    loss = torch.empty((leaves,), device=_cuda(d_all=d_all), dtype=torch.float32)
    dd = torch.empty_like(d_all)
    _launch("isx_triplet_leaves", d_all.data_ptr(), leaves, k, D, float(margin), 1 if normalized else 0, float(scale_a), float(scale_b),
            loss.data_ptr(), dd.data_ptr())
    return loss, dd


# ---- classification fine-tuning (csrc/classif.hip) ---------------------------------------------------
def _xent_args(logits, labels, scale_dev=None):
    """logits (B, C) float32, labels (B) as int32, the optional 1-element scale_dev; closes with the device check."""
    logits = _f32(logits, "logits", (None, None), "(B, C)")
    labels = _typed(labels, torch.int32, "labels", (logits.size(0),))
    sd_ = scale_dev if scale_dev is None else _f32(_meta(scale_dev, "scale_dev").reshape(-1), "scale_dev", 1)
    _cuda(logits=logits, labels=labels, scale_dev=sd_)
    return logits, labels, sd_


def softmax_xent_rows(logits, labels):
    """Per-row cross-entropy log sum_j exp(z_j) - z_label (isx_softmax_xent_fwd).  Labels must lie in [0, C): the caller's contract -- this wrapper does not
    read the labels back to check them (train.classif_finetune.train_classif checks its label list on the host before the first step); an
    out-of-range label yields a NaN loss and reads nothing out of bounds."""
    logits, labels, _ = _xent_args(logits, labels)
    B, Cc = logits.shape
    rows = torch.empty((B,), device=logits.device, dtype=torch.float32)
    _launch("isx_softmax_xent_fwd", logits.data_ptr(), labels.data_ptr(), B, Cc, rows.data_ptr())
    return rows


def softmax_xent_grad(logits, labels, scale=1.0, scale_dev=None):
    """(softmax(z) - onehot(label)) * scale [* scale_dev[0]]; scale_dev: optional 1-element float32 CUDA tensor (autograd's grad_output)."""
    logits, labels, sd_ = _xent_args(logits, labels, scale_dev)
    B, Cc = logits.shape
    dz = torch.empty_like(logits)
    _launch("isx_softmax_xent_bwd", logits.data_ptr(), labels.data_ptr(), B, Cc, float(scale), _ptr(sd_), dz.data_ptr())
    return dz


def softmax_xent_leaves(logits, labels, leaves, scale_a=1.0, scale_b=1.0):
    """Cross-entropy + gradient of every micro-batch of a step in one launch (isx_softmax_xent_leaves).  logits: (leaves * k, C).
    Returns (per-leaf sum of the row losses (leaves,), gradient rows like logits scaled by scale_a * scale_b)."""
    if leaves <= 0 or _meta(logits, "logits", None, (None, None), "(leaves * k, C)").size(0) % leaves:
        raise _lib.IsxError("softmax_xent_leaves: %d rows do not split into %d equal leaves" % (logits.size(0), leaves))
    logits, labels, _ = _xent_args(logits, labels)
    R, Cc = logits.shape
    loss = torch.empty((leaves,), device=logits.device, dtype=torch.float32)
    dz = torch.empty_like(logits)
    _launch("isx_softmax_xent_leaves", logits.data_ptr(), labels.data_ptr(), leaves, R // leaves, Cc, float(scale_a), float(scale_b),
            loss.data_ptr(), dz.data_ptr())
    return loss, dz


def gap_bwd_nhwc(g, H, W):
    """Backward of the whole-map average pool: g (B, C) -> channels-last (B, C, H, W) with every pixel g / (H W) (isx_gap_bwd_nhwc)."""
    g = _f32(g, "g", (None, None))
    B, Cc = g.shape
    dx = _new_nhwc((B, Cc, H, W), _cuda(g=g))
    if B * H * W * Cc and (H * W == 1 or Cc == 1):           # degenerate strides: torch may not lay such a tensor out as (B,H,W,C)
        dx = torch.empty((B, H, W, Cc), device=g.device, dtype=torch.float32).permute(0, 3, 1, 2)
    _launch("isx_gap_bwd_nhwc", g.data_ptr(), B, H, W, Cc, dx.data_ptr())
    return dx


def boxpool_s1_bwd_nhwc(g, H, W, kh, kw):
    """Backward of boxpool_s1_nhwc: g (B, C, H-kh+1, W-kw+1) channels-last -> channels-last (B, C, H, W), every input pixel the sum of the windows
    that cover it (rows, then columns, ascending) divided once by kh * kw (isx_boxpool_s1_bwd_nhwc)."""
    B, Cc, Ho, Wo = _meta(g, "g", torch.float32, (None, None, H - kh + 1, W - kw + 1), "(B, C, H-kh+1, W-kw+1)").shape
    dev = _cuda(g=g)
    gl = g.permute(0, 2, 3, 1)
    if not gl.is_contiguous():
        gl = gl.contiguous()
    dx = torch.empty((B, H, W, Cc), device=dev, dtype=torch.float32)
    _launch("isx_boxpool_s1_bwd_nhwc", gl.data_ptr(), B, Cc, H, W, kh, kw, dx.data_ptr())
    return dx.permute(0, 3, 1, 2)


def linear_wgrad_leaves(dy, x, leaves):
    """dw[l] = dy_l^T x_l for `leaves` consecutive groups of rows, one row-ordered fp32 fma chain per element (isx_linear_wgrad_leaves).
    dy: (leaves * R, N), x: (leaves * R, K) -> (leaves, N, K)."""
    dy = _f32(dy, "dy", (None, None))
    M, N = dy.shape
    x = _f32(x, "x", (M, None), "(dy's rows, K)")
    if leaves <= 0 or M % leaves:
        raise _lib.IsxError("linear_wgrad_leaves: dy %s and x %s do not split into %d equal leaves" % (tuple(dy.shape), tuple(x.shape), leaves))
    K = x.size(1)
    dw = torch.empty((leaves, N, K), device=_cuda(dy=dy, x=x), dtype=torch.float32)
    _launch("isx_linear_wgrad_leaves", dy.data_ptr(), x.data_ptr(), leaves, M // leaves, N, K, dw.data_ptr())
    return dw


def colsum_leaves(x, leaves):
    """Column sums of `leaves` consecutive groups of rows, each over its rows in order (isx_colsum_leaves): x (leaves * R, C) -> (leaves, C)."""
    x = _f32(x, "x", (None, None))
    M, Cc = x.shape
    if leaves <= 0 or M % leaves:
        raise _lib.IsxError("colsum_leaves: %d rows do not split into %d equal leaves" % (M, leaves))
    out = torch.empty((leaves, Cc), device=_cuda(x=x), dtype=torch.float32)
    _launch("isx_colsum_leaves", x.data_ptr(), leaves, M // leaves, Cc, out.data_ptr())
    return out


def head_linear_dgrad(dy, weight):
    """dx = dy W (isx_head_linear_dgrad: the TN kernel on (dy^T, W)).  dy: (M, N); weight: (Np, K) with Np >= N -- a copy the caller has
    zero-padded where N is off the kernel's granule.  The kernel reads dy transposed with the rows padded to a multiple of 64: the (Np, Mp)
    operand is built here, padding classes and rows zero (zero products leave every chain untouched); without either padding it is
    `dy.t().contiguous()`, no zero-fill.  Returns the first M rows, (M, K)."""
    dy, weight = _f32(dy, "dy", (None, None)), _f32(weight, "weight", (None, None))
    M, N = dy.shape
    Np, K = weight.shape
    if Np < N:
        raise _lib.IsxError("head_linear_dgrad: dy %s has more columns than weight %s has rows" % (tuple(dy.shape), tuple(weight.shape)))
    dev = _cuda(dy=dy, weight=weight)
    Mp = (M + 63) // 64 * 64
    if Mp == M and Np == N:
        dyT = dy.t().contiguous()
    else:
        dyT = dy.new_zeros((Np, Mp))
        dyT[:N, :M] = dy.t()
    dx = torch.empty((Mp, K), device=dev, dtype=torch.float32)
    _launch("isx_head_linear_dgrad", dyT.data_ptr(), Mp, Np, weight.data_ptr(), K, dx.data_ptr())
    return dx[:M]


# ---- half-precision filter path (csrc/fast.hip) ----------------------------------------------------
def rows_to_f16(x):
    """(h (B,D) float16, norm2 (B) upper bound of the squared row norm, amax (B) max |x|)."""
    x = _f32(x, "x", (None, None))
    B, D = x.shape
    dev = _cuda(x=x)
    h = torch.empty((B, D), device=dev, dtype=torch.float16)
    n2 = torch.empty((B,), device=dev, dtype=torch.float32)
    am = torch.empty((B,), device=dev, dtype=torch.float32)
    _launch("isx_rows_to_f16", x.data_ptr(), B, D, h.data_ptr(), n2.data_ptr(), am.data_ptr())
    return h, n2, am


def cosine_sim_f16(Qh, Gh, out=None):
    Qh, Gh, M, N, D = _pair(Qh, Gh, torch.float16, ("Qh", "Gh"))
    sim = _sim_out(out, M, N, Qh=Qh, Gh=Gh)
    _launch("isx_cosine_sim_f16", Qh.data_ptr(), M, Gh.data_ptr(), N, D, sim.data_ptr())
    return sim
