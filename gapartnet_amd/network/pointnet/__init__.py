"""The dense PointNet segmentation backbone (reference: network/pointnet/) on the point-MLP kernels of csrc/pointmlp.hip."""
from .pointnet_sem_seg import PointNetSegBackbone  # noqa: F401
from .pointnet_utils import PointNetEncoder, STN3d, STNkd  # noqa: F401
