"""Alias: LovaszSoftmax of lattice_net_amd.losses, the NLLLoss that stands next to it in a training step, and the head that joins them."""
from lattice_net_amd.losses import LovaszSoftmax, NLLLoss, SegmentationLoss, log_softmax  # noqa: F401
