"""MMVID on the AMD Instinct MI355X: PyTorch-ROCm plumbing over hand-written HIP kernels (include/mmvid_hip.h)."""
from ._lib import deterministic, is_deterministic, set_deterministic  # noqa: F401
