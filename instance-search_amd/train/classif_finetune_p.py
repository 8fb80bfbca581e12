"""Parameters of the classification fine-tuning (reference train/classif_finetune_p.py:53-99).  The reference's augmentation
(random_affine_noisy_cv) is OFF by default: the training images are pre-processed once (train_pre_proc = True).  --augment=reference (or
train_pre_proc = False with P.train_trans = utils.image.random_affine_noisy_cv(...)) runs it per batch on the device; any other
user-supplied P.train_trans callable is applied on the host (main() on sets you loaded yourself).  train_bn: the reference enables
BatchNorm learning for batches >= 16; here it stays off by default (the frozen-BatchNorm step runs on the HIP engines), set it to True for
the reference's behaviour on torch autograd."""
from .params import Params

P = Params(cnn_model='AlexNet', feature_size2d=(6, 6), feature_dim=9216,
           train_epochs=50, train_batch_size=32, train_micro_batch=0, train_lr=1e-2, train_momentum=0.9, train_weight_decay=5e-4,
           train_annealing={30: 0.1}, train_loss_avg=True, train_loss_int=10, train_test_int=0, test_descriptor_net=True)
