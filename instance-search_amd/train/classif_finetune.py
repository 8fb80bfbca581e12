"""Global-descriptor approach, pipeline stage 1: the reference's train/classif_finetune.py -- get_embeddings (:82-110), get_class_net
(:113-121), test_classif_net (:25-50) and the fine-tuning of the backbone as a classifier on the instance labels (train_classif :53-78,
main :124-167), whose checkpoint the siamese trainings start from (P.classif_model).  On the GPU the frozen trunk prefix runs once per
mini-batch on the folded HIP trunk, layer4 on isx.suffix.SuffixEngine and pool -> classifier -> cross-entropy on isx.classif_head
(utils/train_general._Stepper); on the CPU, with BatchNorm learning or for AlexNet's classifier the step is plain torch autograd."""
import random

import torch
import torch.nn as nn

from model.custom_modules import CrossEntropyLoss, l2_normalize_rows
from model.siamese import TuneClassif
from utils import fold_batches, log, move_device, tensor, test_print_classif, test_print_descriptor, train_gen
from ._common import (BatchStager, base_model, device_batch_size, label_index, load_weights, make_resident, stage_batch, stage_images,
                      test_transform)
from .classif_finetune_p import P

labels = []   # filled by the entry point once the reference set is listed, then constant


def test_classif_net(net, test_set):
    """(correct, total) classification accuracy of an eval-mode net."""
    trans = test_transform(P)
    if trans is None:
        make_resident(test_set, P.cuda_device)          # get_embeddings needs the set in HBM right after: upload it once, here

    def run(acc, i, is_final, batch):
        correct, total = acc
        with torch.no_grad():
            pred = net(stage_batch(batch, trans, P.cuda_device)).argmax(1).tolist()
        ids = label_index(labels)
        correct += sum(1 for (_, lab, _), p in zip(batch, pred) if ids[lab] == p)
        return correct, total + len(batch)

    return fold_batches(run, (0, 0), test_set, device_batch_size(P, test_set))


def _full_map_pool(net, fmap):
    """True when feature_reduc is exactly one average pool spanning the whole feature map."""
    reduc = list(net.feature_reduc)
    if len(reduc) != 1 or not isinstance(reduc[0], nn.AvgPool2d):
        return False
    ks = reduc[0].kernel_size
    ks = ks if isinstance(ks, tuple) else (ks, ks)
    return tuple(fmap.shape[2:]) == tuple(ks)


def fc7_tap(classifier):
    """classifier[:6] of an AlexNet-style head -- (Dropout, Linear, ReLU, Dropout, Linear, ReLU | Linear(nbClass)), reference
    model/ModelDefinition.py:31-37 -- i.e. the 4096-d "fc7" activation; raises for heads without that layout (ResNet: one Linear)."""
    mods = list(classifier)
    if len(mods) < 7 or not (isinstance(mods[1], nn.Linear) and isinstance(mods[4], nn.Linear) and isinstance(mods[5], nn.ReLU)):
        raise ValueError('fc7 descriptors need an AlexNet-style classifier (Dropout, Linear, ReLU, Dropout, Linear, ReLU, Linear)')
    return nn.Sequential(*mods[:6])


def fc7_size(classifier):
    return fc7_tap(classifier)[4].out_features


def get_embeddings(net, dataset, device, out_size):
    """(len(dataset), out_size) slab of L2-normalised descriptors on `device`.
    P.embeddings_classify False: pooled convolutional features (classifier stripped for the
    pass, restored afterwards); True: the class scores; P.embeddings_fc7 (extension, AlexNet): classifier[:6].  On the GPU the pool + L2 of a batch is
    one fused kernel (`isx_gap_l2`) writing straight into the slab rows."""
    trans = test_transform(P)
    if trans is None:
        make_resident(dataset, P.cuda_device)           # the set goes to HBM once; batches are device-side row gathers
    fc7 = bool(getattr(P, 'embeddings_fc7', False)) and not P.embeddings_classify
    stripped = not P.embeddings_classify and not fc7
    classifier = net.classifier
    if stripped:
        net.classifier = nn.Sequential()
    elif fc7:
        net.classifier = fc7_tap(classifier)                # extension: the 4096-d activation behind the second ReLU (eval mode: Dropout = identity)
    slab = tensor(device, len(dataset), out_size)
    bs = device_batch_size(P, dataset)
    stager = BatchStager(dataset, bs, trans, P.cuda_device)    # resident: row gathers; beyond the HBM budget: double-buffered pinned staging on a copy stream

    def run(slab, i, is_final, batch):
        x = stager.get(i, batch)
        rows = slab[i:i + len(batch)]
        with torch.no_grad():
            if stripped and x.is_cuda and slab.is_cuda:
                fmap = net.features(x)
                if _full_map_pool(net, fmap):
                    from isx import ops
                    ops.gap_l2(fmap.float(), out=rows)        # NCHW or channels-last, consumed in place
                    return slab
                out = net.feature_reduc(fmap)
                out = out.view(out.size(0), -1)
            else:
                out = net(x)
            rows.copy_(l2_normalize_rows(out))
        return slab

    try:
        return fold_batches(run, slab, dataset, bs)
    finally:
        net.classifier = classifier


def get_class_net():
    net = TuneClassif(base_model(P), len(labels), untrained=P.untrained_blocks)
    return move_device(load_weights(net, P.preload_net), P.cuda_device)


def train_classif(net, train_set, testset_tuple, criterion, optimizer, best_score=0):
    """Fine-tune `net` as a classifier of the instance labels (reference :53-78): per epoch the training set is shuffled, a batch is the image
    rows + the label indices, the loss is `criterion` on the class scores."""
    from ._common import augment_keys, is_augmenter
    trans = None if P.train_pre_proc else P.train_trans
    aug = trans if is_augmenter(trans) else None        # the reference's random_affine_noisy_cv: one kernel call per batch, not a host callable per image
    if trans is None or aug is not None:
        make_resident(train_set, P.cuda_device)          # batches become row gathers on the device (augmented: the warp reads the resident rows)
    ids = label_index(labels)
    unknown = sorted(set(lab for _, lab, _ in train_set if lab not in ids))
    if unknown:
        raise ValueError('train_classif: %d training labels are not in the label list (first: %r)' % (len(unknown), unknown[0]))
    if len(labels) > net.feature_size:
        raise ValueError('train_classif: %d labels but the net scores %d classes' % (len(labels), net.feature_size))

    def create_epoch(epoch, train_set, testset_tuple):
        shuffled = list(train_set)                       # the caller's list keeps its order (it may double as the evaluation gallery)
        random.shuffle(shuffled)
        if aug is not None:
            # an image's augmentation is keyed on (P.train_seed, epoch, the item's place in the epoch's list): the same on every rank
            return [item + (i,) for i, item in enumerate(shuffled)], {'epoch': epoch}
        return shuffled, {}

    def create_batch(batch, n, epoch=None):
        if aug is not None:
            keys = augment_keys(P.train_seed, epoch, [item[3] for item in batch], 0)
            x = stage_images([item[0] for item in batch], P.cuda_device, augment=(aug, keys, P.train_seed))
            ids = label_index(labels)
            return [x], [move_device(torch.tensor([ids[item[1]] for item in batch], dtype=torch.int64), P.cuda_device)]
        prep = (lambda im: im) if trans is None else trans
        x = stage_images([prep(im) for im, _, _ in batch], P.cuda_device)
        ids = label_index(labels)
        lab_ids = torch.tensor([ids[lab] for _, lab, _ in batch], dtype=torch.int64)
        return [x], [move_device(lab_ids, P.cuda_device)]

    # same items -> same batch, whenever it is built (nothing is augmented): the step may build the batches of the next mini-batches ahead of
    # their turn (utils/train_general._Stepper._precompute_ahead)
    create_batch.deterministic = trans is None

    def create_loss(t_out, labels_list):
        return criterion(t_out, labels_list[0]), None

    # the loss IS the cross-entropy criterion on the class scores: the step may evaluate pool, classifier and loss of all its micro-batches in
    # one pass (utils/train_general._Stepper._classif_batched -> isx.classif_head), same values per row
    if type(criterion) is CrossEntropyLoss:
        create_loss.cross_entropy = criterion

    return train_gen(train_type(), P, test_print_classif, test_classif_net, net, train_set, testset_tuple, optimizer, create_epoch,
                     create_batch, create_loss, best_score=best_score)


def train_type():
    return P.cnn_model.lower() + ' Classification simple fine-tuning'


def main(train_set, test_train_set, test_set):
    """Training entry (reference :124-167) on already loaded (tensor, label, path) datasets: upfront test (P.test_upfront) -> training
    (P.train) -> evaluation as a descriptor net (P.test_descriptor_net).  Returns (net, best classification score)."""
    from utils.train_general import make_sgd
    from .global_p import flat_feature_sizes
    del labels[:]
    labels.extend(sorted(set(l for _, l, _ in train_set)))
    P.num_classes = len(labels)
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
        score = train_classif(net, train_set, testset_tuple, criterion, optimizer, best_score=score)
        log(P, 'Finished classification training')
    if getattr(P, 'test_descriptor_net', True):
        log(P, 'Testing as descriptor')
        P.feature_dim = P.num_classes if P.embeddings_classify else flat_feature_sizes.get((P.cnn_model.lower(), tuple(P.image_input_size)), P.feature_dim)
        test_print_descriptor(train_type(), P, net, testset_tuple, get_embeddings)
    return net, score


def run(dataset_full=None):
    """The reference's main() (:124-167): the sets come from P.dataset_full (a dataset folder with its `test` sub-folder, or a `synthetic:` spec)."""
    from ._common import load_training_sets
    return main(*load_training_sets(P, dataset_full or P.dataset_full, labels))


if __name__ == '__main__':
    import sys
    from ._common import training_cli
    training_cli(sys.argv[1:], P, run, 'train.classif_finetune')
