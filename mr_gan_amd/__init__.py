"""mr_gan_amd -- MI355X-native feature-matching semi-supervised GAN training path of
Healthcare-Robotics/mr-gan (mr_gan.py), behind the reference's own entry points.

    from mr_gan_amd import mr_gan, dataset, MRGAN
    from mr_gan_amd import Autoencoder, mr_gan_autoencoder      # the autoencoder pre-stage (others/mr_gan_autoencoder.py)
    from mr_gan_amd import RBFSVM                               # the SVM baseline's classifier on the GPU (mr_svm --backend hip)
    from mr_gan_amd import RBFSVMGroup                          # several such problems in one launch set (mr_svm --group-folds)
    from mr_gan_amd import KernelSVM                            # SVC / NuSVC with the RBF or the linear kernel (mr_svm --classifier)
    from mr_gan_amd import KernelSVMGroup                       # several problems of those kinds in one launch set (mr_svm_folds)
    from mr_gan_amd import PCA, pca_scale, mr_gan_pca           # the PCA pre-stage (others/wganlpctsemi.py pcaScale) on the GPU
"""
from mr_gan_amd.data import (select_labeled, standard_scale, synthetic_blobs, synthetic_mreo,  # noqa: F401
                             tiled_permutation)
from mr_gan_amd.autoencoder import Autoencoder, mr_gan_autoencoder  # noqa: F401
from mr_gan_amd.model import MRGAN, MRGANGroup  # noqa: F401
from mr_gan_amd.mr_gan import dataset, mr_gan  # noqa: F401
from mr_gan_amd.svm import KernelSVM, KernelSVMGroup, RBFSVM, RBFSVMGroup  # noqa: F401
from mr_gan_amd.pca import PCA, mr_gan_pca, pca_scale  # noqa: F401

__all__ = ["mr_gan", "dataset", "MRGAN", "MRGANGroup", "Autoencoder", "RBFSVM", "RBFSVMGroup", "KernelSVM", "KernelSVMGroup", "PCA", "pca_scale", "mr_gan_pca", "mr_gan_autoencoder", "synthetic_mreo", "synthetic_blobs", "standard_scale", "select_labeled",
           "tiled_permutation"]
