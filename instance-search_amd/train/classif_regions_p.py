"""Parameters of the sub-region classifier training (reference train/classif_regions_p.py:53-94).  The reference's cv2 augmentation and its
scale_cv are not part of this package: the training images are pre-processed once (train_pre_proc = True) and the second scale is a bicubic
interpolation of the normalised tensor (train_sub_scales: None = the image as is, an int = shorter side to that size), or, with
train_scale_pixels = 'u8', isx.scale's cubic resize of the decoded 8-bit image, normalised afterwards."""
from .params import Params

P = Params(cnn_model='AlexNet', feature_size2d=(6, 6), feature_dim=464,
           train_epochs=50, train_batch_size=32, train_micro_batch=1, train_lr=1e-3, train_momentum=0.9, train_weight_decay=5e-4,
           train_annealing={30: 0.1}, train_loss_avg=True, train_loss_int=10, train_test_int=0, test_descriptor_net=True,
           train_sub_scales=[None, 224])
