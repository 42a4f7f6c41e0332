"""PointNet on 3-D points: the baseline NDT-Net is compared against.

The reference's second arm (ndnet/models/pointnet.py): the same TNets,
per-point MLPs and heads as NDTNet, fed ``[B, N, 3]`` points -- farthest-point
samples of a scan (``ndnet.preprocessing.fps_downsample``) -- instead of
``[B, N, 12]`` normal distributions.  Module tree, constructor arguments and
``state_dict`` keys are the reference's, so its checkpoints and
``tools/train_pointnet.py`` load unchanged:

    PointNetSegmentation / PointNetClassification
      feature_extractor: PointNet
        conv1/conv2/conv3 (+bn1..3), t1: TNet(3), t2: TNet(64)
      conv1.. (the heads of ndtnet.py)

Forward paths, as for the NDT models (``ndnet.models.ndtnet``):
  * eval mode on a gfx950 GPU with no autograd wanted -> the HIP chains of
    ``ndnet.models.pointnet_hip``.  The one difference from NDTNet's sequence:
    the reference clamps the transformed points, ``nan_to_num(t1 p)``
    (pointnet.py:114-117), which is not linear, so t1 is not folded into
    conv1; ``ndnet_pn_transform3_run`` (include/ndnet_nearest.h) applies it to
    the points between TNet(3)'s head and chain B, whose layer 0 is the shared
    conv1.
  * train mode on the GPU -> ``_block`` / ``_block_pool`` / the TNet heads on
    the HIP train kernels, layer for layer as NDTNet.
  * anything else -> ``forward_torch``, the reference op for op.
"""
from __future__ import annotations

import torch
from torch import nn

from .ndtnet import TNet, _HipEval, _block, _block_pool, _conv, _hip_train


class PointNet(nn.Module):
    """Feature extractor (reference pointnet.py:65-135)."""

    points_only = True  # pointnet_hip: conv1 reads 3 columns and stays a shared layer

    def __init__(self, point_dim: int = 3, feature_dim: int = 768) -> None:
        super().__init__()
        self.point_dim = point_dim
        self.feature_dim = feature_dim
        self.conv1 = _conv(point_dim, 64)
        self.conv2 = _conv(64, 128)
        self.conv3 = _conv(128, feature_dim)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(64), nn.BatchNorm1d(128), nn.BatchNorm1d(feature_dim)
        self.t1 = TNet(in_dim=point_dim)
        self.t2 = TNet(in_dim=64)

    def forward(self, x: torch.Tensor, pooled: bool = False):
        """points [B,N,3] -> (features [B,F,N], x_t2 [B,64,N]); ``pooled``:
        (features.amax(dim=2) [B,F], x_t2) -- what the heads use."""
        x = x.transpose(2, 1)                              # [B,3,N]
        t = self.t1(x)                                     # [B,3,3]
        x = torch.bmm(t, x)                                # t . p
        x = torch.nan_to_num(x, nan=0.0)
        x = _block(self.conv1, self.bn1, x, False)         # no ReLU (pointnet.py:120)
        t2 = self.t2(x)                                    # [B,64,64]
        if _hip_train(self.conv2, self.bn2, x):
            from . import train_hip
            x = train_hip.transform_t(x, t2)               # x^T t2 on the HIP GEMM (pointnet.py:124-126)
        else:
            x = torch.bmm(x.transpose(2, 1), t2).transpose(2, 1)
        x_t2 = x
        x = _block(self.conv2, self.bn2, x, False)
        if pooled:
            return _block_pool(self.conv3, self.bn3, x, False), x_t2
        x = _block(self.conv3, self.bn3, x, False)
        return x, x_t2


class _HipEvalPoints(_HipEval):
    """``_HipEval`` for a model whose only input is the points."""

    def _hip_eval_points(self, points: torch.Tensor) -> bool:
        return self._hip_eval(points, points)


class PointNetClassification(_HipEvalPoints, nn.Module):
    """Global classifier (reference pointnet.py:137-167): class probabilities
    [B, num_classes, 1]."""

    def __init__(self, point_dim: int = 3, num_classes: int = 512, feature_dim: int = 768) -> None:
        super().__init__()
        self.point_dim, self.num_classes, self.feature_dim = point_dim, num_classes, feature_dim
        self.feature_extractor = PointNet(point_dim=point_dim, feature_dim=feature_dim)
        self.conv1, self.conv2, self.conv3 = _conv(feature_dim, 512), _conv(512, 256), _conv(256, num_classes)
        self._init_hip()

    def forward_torch(self, points: torch.Tensor) -> torch.Tensor:
        x, _ = self.feature_extractor(points)
        x = x.amax(dim=2, keepdim=True)
        x = torch.relu(self.conv1(x))
        x = torch.relu(self.conv2(x))
        return torch.softmax(self.conv3(x), dim=1)

    def forward(self, points: torch.Tensor) -> torch.Tensor:
        if self._hip_eval_points(points):
            # a cuda eval forward IS the HIP path (a missing library raises); only widths the
            # kernels do not take run the torch composition, as for NDTNetClassification
            from . import pointnet_hip
            if pointnet_hip.supports_classification(self):
                return pointnet_hip.classification_forward(self, points, None)
        return self.forward_torch(points)


class PointNetSegmentation(_HipEvalPoints, nn.Module):
    """Per-point segmentation (reference pointnet.py:169-214): log-probs
    [B,N,C+1]."""

    def __init__(self, point_dim: int = 3, num_classes: int = 16, feature_dim: int = 768) -> None:
        super().__init__()
        self.point_dim, self.num_classes, self.feature_dim = point_dim, num_classes, feature_dim
        self.feature_extractor = PointNet(point_dim=point_dim, feature_dim=feature_dim)
        self.conv1 = _conv(feature_dim + 64, 512)
        self.conv2 = _conv(512, 256)
        self.conv3 = _conv(256, 128)
        self.conv4 = _conv(128, num_classes + 1)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(512), nn.BatchNorm1d(256), nn.BatchNorm1d(128)
        self._init_hip()

    def forward_torch(self, points: torch.Tensor) -> torch.Tensor:
        hip = _hip_train(self.conv1, self.bn1, points)
        x, x_t2 = self.feature_extractor(points, pooled=hip)
        blocks = ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3))
        if hip:
            # as NDTNetSegmentation: conv1 over cat(x_t2, g) as a 64-channel conv with the global
            # feature's term a per-cloud bias
            from . import train_hip
            x = train_hip.seg_conv1(self.conv1, self.bn1, x_t2, x)  # x: the pooled global feature [B,F]
            blocks = blocks[1:]
        else:
            g = x.amax(dim=2, keepdim=True).expand(-1, -1, x_t2.shape[2])
            x = torch.cat((x_t2, g), dim=1)
        for conv, bn in blocks:
            x = _block(conv, bn, x, True)
        x = _block(self.conv4, None, x, False)
        if hip and x.shape[1] <= 32:
            from . import train_hip
            x = train_hip.log_softmax_c(x)
        else:
            x = torch.nn.functional.log_softmax(x, dim=1)
        return x.transpose(2, 1)

    def forward(self, points: torch.Tensor) -> torch.Tensor:
        if self._hip_eval_points(points):
            from . import pointnet_hip
            if pointnet_hip.supports(self):
                return pointnet_hip.segmentation_forward(self, points, None)
        return self.forward_torch(points)
