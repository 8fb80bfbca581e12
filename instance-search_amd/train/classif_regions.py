"""Sub-region classifier approach, pipeline stage 2: get_embeddings (reference train/classif_regions.py:107-132), get_class_net (:135-149),
test_classif_net (:25-51) and the training of the fully convolutional classifier on every sliding window of every scale of an image
(train_classif_subparts :54-102, main :152-200), whose checkpoint the region-descriptor training starts from (P.classif_model of
train.siamese_regions).  Descriptor = the class-score vector at the location whose best class score is highest, L2-normalised.  On the GPU the
frozen trunk prefix runs once per scale and mini-batch on the folded HIP trunk, layer4 on isx.suffix.SuffixEngine and box pool -> classifier ->
cross-entropy over the windows on isx.classif_head (utils/train_general._Stepper._classif_batched); on the CPU, with BatchNorm learning or for
AlexNet's classifier the step is plain torch autograd."""
import random

import torch

from model.custom_modules import CrossEntropyLoss, l2_normalize_rows
from model.siamese import TuneClassif, TuneClassifSub
from utils import log, move_device, tensor, test_print_classif, test_print_descriptor, train_gen
from ._common import (base_model, device_batch_size, fold_shape_buckets, label_index, load_weights, make_resident, scatter_rows, stage_images,
                      test_transform)
from .classif_regions_p import P

labels = []


def _best_location_descriptors(score_map):
    """(B, n_cls, H', W') -> (B, n_cls): libisx `isx_best_location_desc` on the GPU."""
    if score_map.is_cuda:
        from isx import ops
        return ops.best_location_desc(score_map.float())[0]      # NCHW or channels-last, consumed in place
    B, K, Hp, Wp = score_map.shape
    mx = score_map.max(1)[0]                                   # class-max map
    # first maximal index: smallest column, then smallest row in that column
    colmax, row_of_col = mx.max(1)                             # over rows, per column
    col = colmax.max(1)[1]
    row = row_of_col.gather(1, col[:, None])[:, 0]
    picked = score_map[torch.arange(B), :, row, col]
    return l2_normalize_rows(picked)


def test_classif_net(net, test_set):
    """(correct, total): the prediction of an image is the class of its globally highest score over all locations.  The reference walks the set
    one image at a time (:50, "batch size has to be 1 here": sizes may differ); an image's score map does not depend on the batch it rides in,
    so same-shaped images share a launch here (fold_shape_buckets) -- 15 ms of host work per single-image pass otherwise."""
    trans = test_transform(P)
    if trans is None:
        make_resident(test_set, P.cuda_device)          # the queries are classified here AND embedded right after: uploaded once
    ids = label_index(labels)
    correct = [0]

    def run(indices, batch, x):
        with torch.no_grad():
            out = net(x)[0]
            pred = out.max(1)[0].flatten(1).argmax(1)
            flat = out.flatten(2)
            cls = flat[torch.arange(out.size(0), device=out.device), :, pred].argmax(1).tolist()
        correct[0] += sum(1 for (_, lab, _), p in zip(batch, cls) if ids[lab] == p)

    fold_shape_buckets(run, test_set, lambda shape: device_batch_size(P, test_set, shape), stage=(trans, P.cuda_device))
    return correct[0], len(test_set)


def get_embeddings(net, dataset, device, out_size):
    trans = test_transform(P)
    if trans is None:
        make_resident(dataset, P.cuda_device)
    slab = tensor(device, len(dataset), out_size)

    def run(indices, batch, x):
        with torch.no_grad():
            out = net(x)[0]
            scatter_rows(slab, indices, _best_location_descriptors(out))

    # the reference walks one image at a time (images may differ in size); here images are bucketed by shape and every
    # bucket goes through in batches of P.test_batch_size, staged ahead of the trunk (BatchStager)
    fold_shape_buckets(run, dataset, lambda shape: device_batch_size(P, dataset, shape), stage=(trans, P.cuda_device))
    return slab


def get_class_net():
    if P.bn_model:
        bn_model = load_weights(TuneClassif(base_model(P, pretrained=False), len(labels)), P.bn_model)
    else:
        bn_model = base_model(P)
    net = TuneClassifSub(bn_model, len(labels), P.feature_size2d, untrained=P.untrained_blocks)
    return move_device(load_weights(net, P.preload_net), P.cuda_device)


def region_loss(criterion, loss_avg):
    """The reference's loss (:80-98) on the list of class-score maps, one (B, n_cls, H', W') map per scale: every window of an image is a row
    carrying the image's label, `criterion` runs on the rows of a scale (its mean: the mean over each image's windows, the images weighing
    alike), the scales' losses are summed -- and divided by the number of scales when `loss_avg`.  The reference handles B = 1 only.
    labels_list holds ONE tensor, the class index per image (what create_batch builds)."""
    def create_loss(scales_out, labels_list):
        lab = labels_list[0]
        loss = None
        for t_out in scales_out:
            n_cls, loc = t_out.size(1), t_out.size(2) * t_out.size(3)
            rows = t_out.flatten(2).permute(0, 2, 1).reshape(-1, n_cls)            # image-major, then window
            one = criterion(rows, lab.repeat_interleave(loc))
            loss = one if loss is None else loss + one
        if loss_avg:
            loss = loss / len(scales_out)
        return loss, None

    # the loss IS the cross-entropy criterion on the windows of every scale: the step may evaluate pool, classifier and loss of all its
    # micro-batches in one pass per scale (utils/train_general._Stepper._classif_batched -> isx.classif_head), same values per row
    if type(criterion) is CrossEntropyLoss:
        create_loss.region_cross_entropy = criterion
    return create_loss


def _ragged(train_set):
    """True when the images of some scale differ in shape within the set (they cannot share a batch)."""
    return any(len(set(tuple(item[0][j].shape) for item in train_set)) > 1 for j in range(len(train_set[0][0]))) if train_set else False


def train_classif_subparts(net, train_set, testset_tuple, criterion, optimizer, best_score=0):
    """Train `net` on the instance labels of the sub-regions (reference :54-102).  A training item is ([image at scale 0, image at scale 1, ...],
    label, path); per epoch the set is shuffled, a batch is one image stack per scale + one label index per image."""
    trans = None if P.train_pre_proc else P.train_trans          # a list of transforms, one per scale (reference classif_regions_p.py: train_trans)
    ids = label_index(labels)
    unknown = sorted(set(lab for _, lab, _ in train_set if lab not in ids))
    if unknown:
        raise ValueError('train_classif_subparts: %d training labels are not in the label list (first: %r)' % (len(unknown), unknown[0]))
    if len(labels) > net.feature_size:
        raise ValueError('train_classif_subparts: %d labels but the net scores %d classes' % (len(labels), net.feature_size))
    n_sc = len(train_set[0][0]) if train_set else 0
    if any(len(item[0]) != n_sc for item in train_set):
        raise ValueError('train_classif_subparts: every training item needs the same number of scales')
    if trans is not None and (not isinstance(trans, (list, tuple)) or len(trans) != n_sc or not all(callable(t) for t in trans)):
        raise ValueError('train_classif_subparts: with P.train_pre_proc False, P.train_trans must be a list of %d callables, one per scale' % n_sc)
    if trans is None and not _ragged(train_set):
        # one resident block per scale; train._common keeps the four most recent blocks (two scales + gallery + queries): with more scales the
        # oldest block is dropped and stage_images stacks that scale's batches on the host again (same values)
        for j in range(n_sc):
            make_resident([(item[0][j], item[1], item[2]) for item in train_set], P.cuda_device)     # batches become row gathers on the device

    def create_epoch(epoch, train_set, testset_tuple):
        shuffled = list(train_set)                       # the caller's list keeps its order
        random.shuffle(shuffled)
        return shuffled, {}

    def create_batch(batch, n):
        prep = [(lambda im: im)] * n_sc if trans is None else trans
        xs = [stage_images([prep[j](item[0][j]) for item in batch], P.cuda_device) for j in range(n_sc)]
        ids = label_index(labels)
        lab_ids = torch.tensor([ids[lab] for _, lab, _ in batch], dtype=torch.int64)
        return xs, [move_device(lab_ids, P.cuda_device)]

    create_batch.deterministic = trans is None           # same items -> same batch (utils/train_general._Stepper._precompute_ahead)
    create_loss = region_loss(criterion, P.train_loss_avg)
    return train_gen(train_type(), P, test_print_classif, test_classif_net, net, train_set, testset_tuple, optimizer, create_epoch,
                     create_batch, create_loss, best_score=best_score)


def train_type():
    return P.cnn_model.lower() + ' Classification sub-regions'


def main(train_set, test_train_set, test_set):
    """Training entry (reference :152-200) on already loaded sets -- train_set: ([image per scale], label, path) items, the test sets: (image,
    label, path): upfront test (P.test_upfront) -> training (P.train) -> evaluation as a descriptor net (P.test_descriptor_net).  Returns
    (net, best classification score)."""
    from utils.train_general import make_sgd
    del labels[:]
    labels.extend(sorted(set(l for _, l, _ in train_set)))
    P.num_classes = len(labels)
    if _ragged(train_set):
        # images of different sizes cannot share a launch: one image per micro-batch (the reference's "has to be 1"), trunk inside the step
        P.train_micro_batch = 1
        P.train_trunk_per_minibatch = False
    net = get_class_net()
    optimizer = make_sgd((p for p in net.parameters() if p.requires_grad), P.train_lr, P.train_momentum, P.train_weight_decay)
    criterion = CrossEntropyLoss(size_average=P.train_loss_avg)
    testset_tuple = (test_set, test_train_set)
    score = 0
    if getattr(P, 'test_upfront', True):
        log(P, 'Upfront testing of classification model')
        score = test_print_classif(train_type(), P, net, testset_tuple, test_classif_net)
    if getattr(P, 'train', True):
        log(P, 'Starting classification training')
        score = train_classif_subparts(net, train_set, testset_tuple, criterion, optimizer, best_score=score)
        log(P, 'Finished classification training')
    if getattr(P, 'test_descriptor_net', True):
        log(P, 'Testing as descriptor')
        P.feature_dim = P.num_classes
        test_print_descriptor(train_type(), P, net, testset_tuple, get_embeddings)
    return net, score


def scale_image(im, size):
    """A normalised (3, H, W) image with its shorter side brought to `size` (None: as is): bicubic interpolation of the normalised tensor.  The
    reference resizes the decoded 8-bit image with OpenCV before normalising (utils/image.py scale_cv): not the same pixels."""
    if size is None:
        return im
    H, W = im.shape[1], im.shape[2]
    if min(H, W) == size:
        return im
    h, w = (size, max(1, int(round(W * size / float(H))))) if H <= W else (max(1, int(round(H * size / float(W)))), size)
    return torch.nn.functional.interpolate(im.unsqueeze(0), size=(h, w), mode='bicubic', align_corners=False)[0].contiguous()


def scale_image_u8(im_u8, size):
    """A raw (H, W, 3) uint8 image with its shorter side brought to `size` (None: as is), as the reference's scale_cv does it: the cubic resize
    of the 8-bit image (isx.scale, the pixels defined in include/isx_scale.h), on the device when P.cuda_device >= 0 and on the host otherwise
    -- the same bytes."""
    from isx import scale
    if size is None:
        return im_u8
    hw = scale.short_side_size(im_u8.shape[0], im_u8.shape[1], size)
    if hw == tuple(im_u8.shape[:2]):
        return im_u8
    if P.cuda_device >= 0:
        with torch.cuda.device(P.cuda_device):
            return scale.resize_cubic_u8(im_u8.unsqueeze(0).cuda(), hw)[0].cpu()
    return scale.resize_cubic_u8_host(im_u8.unsqueeze(0), hw)[0]


def multi_scale_items(train_set, scales, pixels='normalised'):
    """(image, label, path) -> ([image at every scale of `scales`], label, path).  pixels='normalised' (the default): raw uint8 images are
    normalised first and the fp32 tensor is interpolated (scale_image).  pixels='u8': the raw uint8 image is resized (scale_image_u8) and
    normalised afterwards, the reference's order; images that are not raw uint8 are refused in that mode."""
    from ._common import normalise_u8_batch

    def norm(im):
        return normalise_u8_batch(im.unsqueeze(0), -1)[0] if im.dtype == torch.uint8 else im

    if pixels == 'u8':
        for im, _, path in train_set:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                raise ValueError("pixels='u8' needs raw (H,W,3) uint8 images, got %s %s for %s" % (tuple(im.shape), im.dtype, path))
        items = [([norm(scale_image_u8(im, s)) for s in scales], lab, path) for im, lab, path in train_set]
    elif pixels == 'normalised':
        items = [([scale_image(norm(im), s) for s in scales], lab, path) for im, lab, path in train_set]
    else:
        raise ValueError("pixels must be 'normalised' or 'u8', got %r" % (pixels,))
    for ims, _, path in items:
        shapes = [tuple(im.shape) for im in ims]
        if len(set(shapes)) != len(shapes):               # e.g. scales (None, 224) on a 224-pixel image: the same windows would be trained on twice
            raise ValueError('scales %r give the same image twice for %s (%s)' % (list(scales), path, shapes))
    return items


def run(dataset_full=None):
    """The reference's main() (:152-200): the sets come from P.dataset_full (a dataset folder with its `test` sub-folder, or a `synthetic:` spec),
    every training image at the scales of P.train_sub_scales (None: as is, an int: shorter side to that size; reference classif_regions_p.py:
    [identity, scale_cv(224)])."""
    from ._common import is_augmenter, load_training_sets
    if is_augmenter(getattr(P, 'train_trans', None)):
        # not built: the reference resizes every scale at load and warps each stored scale per batch (one isx_affine_noisy_u8 call per scale on
        # the uint8 scales of pixels='u8' would do it); the message below is older than that reading of the reference
        raise NotImplementedError('train.classif_regions: augmentation is not supported here -- the per-scale transform lists of the reference '
                                  '(classif_regions_p.py) resize after the warp, which isx_affine_noisy_u8 does not do; run with --augment=off')
    train_set, test_train_set, test_set = load_training_sets(P, dataset_full or P.dataset_full, labels)
    scales = list(getattr(P, 'train_sub_scales', None) or [None, 224])
    # P.train_scale_pixels (--scale-pixels): 'u8' resizes the decoded 8-bit image and normalises afterwards, as the reference does
    return main(multi_scale_items(train_set, scales, getattr(P, 'train_scale_pixels', None) or 'normalised'), test_train_set, test_set)


if __name__ == '__main__':
    import sys
    from ._common import training_cli
    training_cli(sys.argv[1:], P, run, 'train.classif_regions')
