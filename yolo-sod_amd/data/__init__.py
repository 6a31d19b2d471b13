from .nv12 import NV12_COEF, NV12_MATRICES, NV12Frame  # noqa: F401
