"""Alias: LovaszSoftmax of lattice_net_amd.losses, and the NLLLoss that stands next to it in a training step."""
from lattice_net_amd.losses import LovaszSoftmax, NLLLoss  # noqa: F401
