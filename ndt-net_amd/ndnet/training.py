"""The training step of tools/train.py, on the HIP path.

Reference: tools/train.py:16-92 (run_one_epoch) and :95-208 (driver).  Per
batch: ndt_preprocessing with labels (the labelled NDT path: per-voxel class
histogram + first-max argmax, one-hot of num_classes + 1) -> NDTNetSegmentation
forward in train mode (BatchNorm batch statistics, torch autograd) -> loss ->
backward -> Adam step.  With more than one process the model is wrapped in
DistributedDataParallel: one process per GPU, gradients all-reduced over RCCL
(backend "nccl") in buckets that overlap the backward pass; BatchNorm stays
per-rank (the reference has no SyncBN).  Gradients are 3.37 M fp32 = 13.5 MB
per step at F = 768: ``bucket_cap_mb`` 4 gives four all-reduces, the first
starting while the seg head's backward still runs.

The reference's defects on this path are fixed, not reproduced:
  * the loss: train.py:72 calls cross_entropy(pred [B,N,C+1], gt) -- dim 1
    (points) taken as the class dim -- on log-probabilities; here the NLL of
    the one-hot target over the class dim of the model's log-softmax output;
  * backward/step ran in val/test too (train.py:74-81): only in train mode;
  * loss.item() on a float (train.py:77-78) raised; the LR decay
    ``epoch+1 % 20`` was dead code (train.py:54): halved every 20 epochs.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def segmentation_loss(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """Mean NLL of one-hot ``gt`` [B,N,C+1] under log-probs ``pred`` [B,N,C+1]
    (= cross_entropy over the class dim of the pre-log-softmax logits).  On the
    GPU, for the model's output (the transposed view of a [B,C+1,N] tensor),
    one HIP reduction and one HIP gradient launch (train_hip.nll_onehot)
    instead of torch's ~8 elementwise / reduce launches."""
    if (pred.is_cuda and gt.is_cuda and pred.dtype == torch.float32 and gt.dtype == torch.float32
            and pred.dim() == 3 and pred.shape == gt.shape and pred.shape[-1] <= 32
            and pred.transpose(1, 2).is_contiguous()
            and gt.is_contiguous()):
        from .models import train_hip
        return train_hip.nll_onehot(pred.transpose(1, 2), gt)
    return -(gt * pred).sum(dim=-1).mean()


def _hist_on_hip(pred: torch.Tensor, hist: torch.Tensor) -> bool:
    """The point-level kernels take the model's output as it stands: the
    [B,N,C+1] view of contiguous [B,C+1,N] fp32 log-probs, C + 1 <= 32, and a
    contiguous int32 histogram of the same shape on the same GPU."""
    return (pred.is_cuda and hist.is_cuda and pred.device == hist.device and pred.dtype == torch.float32
            and hist.dtype == torch.int32 and pred.dim() == 3 and pred.shape == hist.shape
            and pred.numel() > 0 and pred.shape[-1] <= 32
            and pred.transpose(1, 2).is_contiguous() and hist.is_contiguous())


def point_loss_torch(pred: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """``point_loss`` composed from torch ops (any device): the definition."""
    h = hist.to(pred.dtype)
    terms = torch.where(hist != 0, h * pred, torch.zeros((), dtype=pred.dtype, device=pred.device))
    w = hist.sum(dtype=torch.int64)
    return -terms.sum() / w.clamp(min=1).to(pred.dtype)  # W == 0: no term, loss 0


def point_loss(pred: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """The point-level loss: ``-(1/W) sum_{b,r,c} hist[b,r,c] pred[b,r,c]``
    with ``W = hist.sum()`` -- the mean NLL of every counted point under the
    log-probs ``pred`` [B,k,C+1] of the ND row it was folded into, ``hist``
    [B,k,C+1] being the rows' class histograms (``segment.row_histogram``).  A
    zero count contributes nothing, whatever its log-prob (``0 * -inf`` is 0
    here), and an empty histogram gives 0.  With rows filled to the nearest
    ND this is exactly the mean NLL of what ``segment.segment_points`` would
    predict for every labelled point, and rows past a cloud's survivors
    carry no weight.  On the GPU, under the conditions of
    ``segmentation_loss``, one HIP reduction and one HIP gradient launch
    (train_hip.nll_hist); otherwise the torch composition."""
    if _hist_on_hip(pred, hist):
        from .models import train_hip
        return train_hip.nll_hist(pred.transpose(1, 2), hist)
    return point_loss_torch(pred, hist)


def point_accuracy_tensor(pred: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """The fraction of the counted points whose ND row predicts their class:
    ``sum_{b,r} hist[b, r, argmax pred[b, r]] / hist.sum()`` (first maximum,
    NaN as a maximum; 0 for an empty histogram), a 0-d float32 tensor on pred's
    device without a host sync.  One HIP kernel under ``point_loss``'s
    conditions (ndnet_tr_hist_match_cm), else torch ops."""
    if _hist_on_hip(pred, hist):
        from . import _lib
        Bn, N, C = pred.shape
        ctr = torch.zeros(3, device=pred.device, dtype=torch.int64)
        acc = torch.empty((), device=pred.device, dtype=torch.float32)
        _lib.check(_lib.lib().ndnet_tr_hist_match_cm(pred.data_ptr(), hist.data_ptr(), Bn, C, N, ctr.data_ptr(),
                                                     acc.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "ndnet_tr_hist_match_cm")
        return acc
    matched = hist.gather(-1, pred.argmax(dim=-1, keepdim=True)).sum(dtype=torch.int64)
    w = hist.sum(dtype=torch.int64)
    return torch.where(w > 0, matched.float() / w.clamp(min=1).float(), torch.zeros((), device=pred.device))


class HipAdam(torch.optim.Adam):
    """``torch.optim.Adam(..., capturable=True, fused=True)`` -- the graphed
    step's optimizer -- with the update of every parameter on one HIP launch
    per 32 tensors (``ndnet_tr_adam``, include/ndnet_train.h: torch's fused
    order of operations, the step counts and moments kept in torch's state
    layout, so ``state_dict`` round-trips).  torch's fused kernel took two
    ~46 us launches per step on the 3.37 M parameters (r05p trace).  Falls
    back to torch's own step for anything the kernel does not cover (amsgrad,
    maximize, non-float32 or sparse gradients, a closure)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0) -> None:
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True, fused=True)

    @staticmethod
    def _covered(group, ps) -> bool:
        lr = group["lr"]
        return (not group.get("amsgrad") and not group.get("maximize") and not group.get("differentiable")
                and not group.get("decoupled_weight_decay", False)
                and torch.is_tensor(lr) and lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1
                and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and not p.grad.is_sparse
                        and p.grad.dtype == torch.float32 and p.grad.is_contiguous() for p in ps))

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            return super().step(closure)
        groups = [(g, [p for p in g["params"] if p.grad is not None]) for g in self.param_groups]
        if not all(self._covered(g, ps) for g, ps in groups):
            return super().step()
        import ctypes
        from . import _lib
        for group, ps in groups:
            if not ps:
                continue
            for p in ps:
                st = self.state[p]
                if len(st) == 0:  # torch's capturable fused initial state
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            n = len(ps)
            arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
            b1, b2 = group["betas"]
            rc = _lib.lib().ndnet_tr_adam(
                n, arr(ps), arr([p.grad for p in ps]), arr([self.state[p]["exp_avg"] for p in ps]),
                arr([self.state[p]["exp_avg_sq"] for p in ps]), arr([self.state[p]["step"] for p in ps]),
                (ctypes.c_int64 * n)(*[p.numel() for p in ps]), group["lr"].data_ptr(), float(b1), float(b2),
                float(group["eps"]), float(group["weight_decay"]), torch.cuda.current_stream(ps[0].device).cuda_stream)
            _lib.check(rc, "ndnet_tr_adam")
        return None


def accuracy_tensor(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """Fraction of NDs whose argmax class matches (train.py:84-87), as a 0-d
    tensor on pred's device (no host sync).  On the GPU one HIP kernel
    (ndnet_tr_argmax_match: torch's reduction kernels took ~83 us per argmax)."""
    if (pred.is_cuda and gt.is_cuda and pred.shape == gt.shape and pred.numel() > 0
            and pred.dtype == torch.float32 and gt.dtype == torch.float32):
        # the kernel indexes gt with pred's rows and columns: only for equal shapes
        from . import _lib
        g = gt.contiguous()
        cols = pred.shape[-1]
        rows = pred.numel() // cols
        st = torch.cuda.current_stream().cuda_stream
        if pred.dim() == 3 and cols <= 32 and not pred.is_contiguous() and pred.transpose(1, 2).is_contiguous():
            # the model's [B,N,C] view of its [B,C,N] log-probs: read in place, the
            # fraction written by the kernel's last workgroup
            Bn, N, C = pred.shape
            ctr = torch.zeros(2, device=pred.device, dtype=torch.int32)
            acc = torch.empty((), device=pred.device, dtype=torch.float32)
            _lib.check(_lib.lib().ndnet_tr_argmax_match_cm(pred.data_ptr(), g.data_ptr(), Bn, C, N, ctr.data_ptr(),
                                                           acc.data_ptr(), st), "ndnet_tr_argmax_match_cm")
            return acc
        else:
            cnt = torch.zeros((), device=pred.device, dtype=torch.int32)
            p = pred.contiguous()
            _lib.check(_lib.lib().ndnet_tr_argmax_match(p.data_ptr(), g.data_ptr(), rows, cols, cnt.data_ptr(), st),
                       "ndnet_tr_argmax_match")
        return cnt.float() / rows
    return (pred.argmax(dim=-1) == gt.argmax(dim=-1)).float().mean()


def accuracy(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """Fraction of NDs whose argmax class matches (train.py:84-87)."""
    return accuracy_tensor(pred, gt).item()


def lr_for_epoch(base_lr: float, epoch: int) -> float:
    """The intended schedule of train.py:53-57: halve every 20 epochs."""
    return base_lr * 0.5 ** ((epoch + 1) // 20)


class Trainer:
    """One model + Adam (+ DDP when a process group is active).

    ``graphs=True`` (one GPU, no DDP): ``step`` replays the whole training step
    -- labelled NDT, train forward, loss, backward, Adam -- as one HIP graph per
    input shape (``GraphedTrainStep``).  The optimizer is then Adam's fused,
    capturable form (``HipAdam``: its update on the HIP kernel) with the
    learning rate in a device tensor, so ``set_epoch`` still takes effect
    inside the graph.

    ``loss="nds"`` (default): every ND row is trained against the hard class
    of its voxel, the NLL of the labelled NDT run's one-hot
    (``segmentation_loss``).  ``loss="points"``: the objective the evaluation
    counts (``segment.iou`` is per point) -- after the labelled NDT run the
    points' rows (``NdtPlan.point_rows`` with ``point_fill``) and labels give
    every row its class histogram (``segment.row_histogram``, labels equal to
    ``ignore_label`` left out) and the step minimises ``point_loss``, returning
    it with ``point_accuracy_tensor``.  With ``point_fill="nearest"`` that is
    exactly the mean NLL of what ``segment.segment_points`` would predict for
    every labelled point of the batch; rows past a cloud's survivors carry no
    weight under either fill.  ``point_fill="none"`` leaves out the points of
    pruned NDs and the ``n % 8`` tail.

    ``step`` and ``step_graphed`` take the labels as a one-hot float tensor
    ``[B, n, C + 1]`` or as integer class ids ``[B, n]`` (the same bits either
    way), and ``counts`` for a ragged batch (``collate_padded``): cloud ``b``
    is its first ``counts[b]`` points, the padding of points and labels may
    hold anything.

    DDP needs nothing more for the point loss: it is a per-rank scalar,
    normalised by the rank's own ``W``, and the gradients are averaged over
    the ranks as before.

    ``augment`` (an ``ndnet.augment.Augment``): every training step -- eager or
    captured, never the eval step -- first augments its points, class ids and
    counts on the GPU; the labelled NDT run and the point loss then see the
    augmented batch.  With ``drop > 0`` the step runs the ragged path on the
    augmentation's device counts; with ``drop == 0`` and no ``counts`` it stays
    on the fixed-size path.  A ``stream`` left open becomes the rank, so every
    DDP rank draws its own augmentations from one seed."""

    LOSSES = ("nds", "points")
    POINT_FILLS = ("nearest", "none")

    def __init__(self, model: torch.nn.Module, lr: float, num_nds: int, num_classes: int,
                 device: torch.device, ddp: Optional[bool] = None, bucket_cap_mb: float = 4.0,
                 graphs: bool = False, loss: str = "nds", point_fill: str = "nearest",
                 ignore_label: int = -1, augment=None) -> None:
        if loss not in self.LOSSES:  # (checked before any GPU work)
            raise ValueError(f"loss must be one of {self.LOSSES}, got {loss!r}")
        if augment is not None:
            from .augment import Augment
            if not isinstance(augment, Augment):
                raise ValueError(f"augment must be an ndnet.augment.Augment, got {type(augment).__name__}")
        self.augment = augment
        if point_fill not in self.POINT_FILLS:
            raise ValueError(f"point_fill must be one of {self.POINT_FILLS}, got {point_fill!r}")
        self.loss, self.point_fill, self.ignore_label = loss, point_fill, int(ignore_label)
        import torch.distributed as dist
        self.model = model.to(device)
        self.device = device
        self.num_nds, self.num_classes = int(num_nds), int(num_classes)
        self.base_lr = float(lr)
        if ddp is None:
            ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if graphs and (ddp or device.type != "cuda"):
            raise ValueError("graphs=True needs one GPU and no DDP (the gradient all-reduce is not captured)")
        self.graphs = bool(graphs)
        self._graphed: dict = {}
        if ddp:
            from torch.nn.parallel import DistributedDataParallel as DDP
            ids = [device.index if device.index is not None else torch.cuda.current_device()] \
                if device.type == "cuda" else None
            self.net = DDP(self.model, device_ids=ids, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True)
        else:
            self.net = self.model
        if self.graphs:
            self.opt = HipAdam(self.model.parameters(), lr=torch.tensor(self.base_lr, device=device))
        else:
            self.opt = torch.optim.Adam(self.model.parameters(), lr=self.base_lr)
        if augment is not None:
            augment.resolve_stream()  # (after the DDP set-up: the rank by default)

    def set_epoch(self, epoch: int) -> None:
        for g in self.opt.param_groups:
            if torch.is_tensor(g["lr"]):
                g["lr"].fill_(lr_for_epoch(self.base_lr, epoch))  # the captured step reads it
            else:
                g["lr"] = lr_for_epoch(self.base_lr, epoch)

    def step_on_nds(self, pcl: torch.Tensor, covs: torch.Tensor, gt: torch.Tensor,
                    train: bool = True, hist: Optional[torch.Tensor] = None) -> Tuple[float, float]:
        """Forward (+ backward + Adam step when ``train``) on preprocessed NDs:
        ``pcl`` [B,k,3], ``covs`` [B,k,9], one-hot ``gt`` [B,k,C+1].  With
        ``hist`` (the rows' class histograms, int32 [B,k,C+1]) the loss and the
        accuracy are the point-level ones and ``gt`` is not read."""
        if hist is None:
            loss_fn, acc_fn, target = segmentation_loss, accuracy_tensor, gt
        else:
            loss_fn, acc_fn, target = point_loss, point_accuracy_tensor, hist
        if train:
            self.model.train()
            pred = self.net(pcl, covs)
            loss = loss_fn(pred, target)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            self.opt.step()
        else:
            self.model.eval()
            with torch.no_grad():
                pred = self.model(pcl, covs)
                loss = loss_fn(pred, target)
        return loss.item(), acc_fn(pred.detach(), target).item()

    def nds_and_targets(self, points: torch.Tensor, gt_points: torch.Tensor, counts=None, *, augment: bool = False):
        """The labelled NDT run of a batch and the step's target: ``(pcl, covs,
        gt, hist)`` with ``hist`` None for ``loss="nds"``, else the rows' class
        histograms from the points' rows and labels (all on the GPU; the eager
        and the captured step both run this).  ``augment=True`` (the training
        steps) puts the trainer's ``Augment``, if it has one, in front: its
        points, ids and counts take the inputs' place."""
        from .preprocessing.ndtnet_preprocessing import check_class_ids, check_counts, class_ids, ndt_preprocessing
        check_class_ids(gt_points, points)
        if augment and self.augment is not None:
            if counts is not None:
                check_counts(counts, points.shape[0], points.shape[1])
            pts = points.to(device=self.device, dtype=torch.float32)
            points, gt_points, kept = self.augment(pts, class_ids(gt_points, self.device), counts)
            if counts is not None or self.augment.drop > 0:
                counts = kept  # (else every cloud is whole: the fixed-size path)
        if self.loss == "nds":
            pcl, covs, gt = ndt_preprocessing(self.num_nds, points.to(self.device), gt_points.to(self.device),
                                              self.num_classes, counts=counts)
            return pcl, covs, gt, None
        from . import segment
        pts = points.to(device=self.device, dtype=torch.float32).contiguous()
        labels = class_ids(gt_points, self.device)  # ids as they come, or ndnet_row_argmax of a one-hot
        pcl, covs, gt = ndt_preprocessing(self.num_nds, pts, labels, self.num_classes, counts=counts)
        plan = ndt_preprocessing.last_plan
        rows = plan.point_rows(pts, ndt_preprocessing.last_rows, self.num_nds, self.point_fill,
                               counts=ndt_preprocessing.last_counts)
        hist = segment.row_histogram(rows, labels, self.num_nds, self.num_classes + 1, self.ignore_label)
        return pcl, covs, gt, hist

    def step(self, points: torch.Tensor, gt_points: torch.Tensor, train: bool = True,
             counts=None) -> Tuple[float, float]:
        """One batch of raw clouds: ``points`` [B,n,3], ``gt_points`` one-hot
        [B,n,C+1] or integer class ids [B,n], ``counts`` the per-cloud point
        counts of a ragged batch -> the labelled NDT path on the GPU (and, for
        ``loss="points"``, the rows' histograms) -> step_on_nds (or, with
        ``graphs``, a replay of the captured step)."""
        if train and self.graphs:
            loss, acc = self.step_graphed(points, gt_points, counts)
            return loss.item(), acc.item()
        pcl, covs, gt, hist = self.nds_and_targets(points, gt_points, counts, augment=train)
        return self.step_on_nds(pcl, covs, gt, train, hist)

    def _graph_for(self, points_shape, gt_shape, ragged: bool = False) -> "GraphedTrainStep":
        key = (tuple(points_shape), tuple(gt_shape)) + ((True,) if ragged else ())
        g = self._graphed.get(key)
        if g is None:
            gt_width = gt_shape[-1] if len(gt_shape) == 3 else None  # None: integer class ids
            g = self._graphed[key] = GraphedTrainStep(self, points_shape, gt_width, ragged=ragged)
        return g

    def step_graphed(self, points: torch.Tensor, gt_points: torch.Tensor,
                     counts=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """A training step as a graph replay; returns (loss, accuracy) as device
        scalars, without synchronising.  Passing the graph's own input buffers
        (``graph_inputs``) skips the copies into them.  ``gt_points`` one-hot
        or integer ids, as ``step`` takes them; with ``counts`` the step is
        captured once with a static count buffer and serves any counts."""
        from .preprocessing.ndtnet_preprocessing import check_class_ids, check_counts
        check_class_ids(gt_points, points)
        if counts is not None:
            check_counts(counts, points.shape[0], points.shape[1])
        return self._graph_for(points.shape, gt_points.shape, counts is not None)(points, gt_points, counts)

    def graph_inputs(self, points_shape, gt_shape, counts: bool = False):
        """The static (points, gt) buffers the captured step of this shape
        reads -- gt float one-hot for a 3-D ``gt_shape``, int32 class ids for
        ``[B, n]`` -- and, with ``counts=True``, the int32 ``[B]`` count buffer
        of the ragged step as a third: a loader can fill them in place (e.g. a
        pinned-host copy) and pass them to ``step_graphed`` with no
        device-to-device copy."""
        g = self._graph_for(points_shape, gt_shape, bool(counts))
        return (g.s_points, g.s_gt, g.s_counts) if counts else (g.s_points, g.s_gt)


def _capture_step(model: torch.nn.Module, opt, dev, body, counters=(), warmup: int = 3):
    """``body()`` -- a whole training step on static buffers -- captured into
    one HIP graph: ``(graph, body's return value)``.  Capture needs the step's
    lazy state to exist (library handles, MIOpen's algorithm choices, the
    gradients and Adam's moments), so ``warmup`` steps run eagerly on a side
    stream first; the parameters, the buffers, the optimizer state and the
    device ``counters`` (the step tensors of an ``Augment`` or a
    ``RandomSample``) are snapshotted before them and restored after the
    capture, so the first replay is the trainer's first step and draw 0."""
    with torch.no_grad():
        params = [p.detach().clone() for p in model.parameters()]
        bufs = [b.detach().clone() for b in model.buffers()]
        saved = {p: {k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for p, st in opt.state.items()}
        steps = [c.clone() for c in counters]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(max(1, int(warmup))):
            opt.zero_grad(set_to_none=True)
            body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    with torch.no_grad():
        for p, s in zip(model.parameters(), params):
            p.copy_(s)
        for b, s in zip(model.buffers(), bufs):
            b.copy_(s)
        for p, st in opt.state.items():
            before = saved.get(p, {})
            for k, v in st.items():
                if torch.is_tensor(v):
                    if k in before:
                        v.copy_(before[k])
                    else:
                        v.zero_()  # a fresh moment / step count
        for c, s in zip(counters, steps):
            c.copy_(s)  # the warm-up's draws are rolled back
    torch.cuda.synchronize(dev)
    return graph, out


def _replay_step(step, points: torch.Tensor, gt_points: torch.Tensor, counts) -> Tuple[torch.Tensor, torch.Tensor]:
    """The inputs into ``step``'s static buffers (unless they are those
    buffers) and one replay of its graph: ``(loss, accuracy)``."""
    if (counts is not None) != (step.s_counts is not None):
        raise ValueError("counts go with a step captured with ragged=True, and only with it")
    # the replay does not run Python: flip the mode here, so an eval forward
    # after it re-folds the updated weights (NDTNetSegmentation.train)
    step.tr.model.train()
    if points.data_ptr() != step.s_points.data_ptr():
        step.s_points.copy_(points, non_blocking=True)
    if gt_points.data_ptr() != step.s_gt.data_ptr():
        step.s_gt.copy_(gt_points, non_blocking=True)
    if counts is not None and not (torch.is_tensor(counts) and counts.data_ptr() == step.s_counts.data_ptr()):
        step.s_counts.copy_(torch.as_tensor(counts).to(torch.int32), non_blocking=True)
    step.graph.replay()
    return step.loss, step.acc


class GraphedTrainStep:
    """tools/train.py:67-81 for one input shape, captured once and replayed:
    ndt_preprocessing with labels (HIP) -> train-mode forward -> NLL loss ->
    backward -> fused Adam, with the inputs copied into static buffers.
    With ``loss="points"`` the points' rows and the rows' class histograms
    follow the NDT run inside the graph.  The label buffer ``s_gt`` is float
    one-hot (``gt_width`` columns) or, with ``gt_width=None``, int32 class ids;
    ``ragged=True`` adds the int32 ``[B]`` count buffer ``s_counts``, which the
    kernels read at replay: one graph serves any counts.

    Capture needs the step's lazy state to exist (cuBLAS-style handles,
    MIOpen's algorithm choices, the gradients and Adam's moments), so a few
    steps run eagerly on a side stream first; the parameters, buffers and
    optimizer state are snapshotted before them and restored after the
    capture, so the first replay is the trainer's first step.  The trainer's
    ``Augment`` runs inside the graph; its step counter is snapshotted and
    restored with the weights, so the first replay is draw 0 and every replay
    draws anew."""

    def __init__(self, trainer: Trainer, points_shape, gt_width: Optional[int], warmup: int = 3,
                 ragged: bool = False) -> None:
        tr = self.tr = trainer
        dev = tr.device
        self.s_points = torch.zeros(tuple(points_shape), dtype=torch.float32, device=dev)
        if gt_width is None:  # integer class ids (class 0 for the warm-up steps)
            self.s_gt = torch.zeros(tuple(points_shape[:2]), dtype=torch.int32, device=dev)
        else:
            self.s_gt = torch.zeros(tuple(points_shape[:2]) + (int(gt_width),), dtype=torch.float32, device=dev)
            self.s_gt[..., 0] = 1.0
        # ragged: the kernels read the counts on the device at replay, so one
        # graph serves any counts; warm-up and capture run on whole clouds
        self.s_counts = torch.full((points_shape[0],), points_shape[1], dtype=torch.int32, device=dev) \
            if ragged else None
        # a non-degenerate cloud for the warm-up steps (zeros would be one voxel)
        gen = torch.Generator(device=dev).manual_seed(0)
        self.s_points.copy_(torch.rand(self.s_points.shape, device=dev, generator=gen) * 20 - 10)
        counters = [tr.augment.step_tensor(dev)] if tr.augment is not None else []
        self.graph, (self.loss, self.acc) = _capture_step(tr.model, tr.opt, dev, self._body, counters, warmup)

    def _body(self):
        tr = self.tr
        pcl, covs, gt, hist = tr.nds_and_targets(self.s_points, self.s_gt, self.s_counts, augment=True)
        tr.model.train()
        pred = tr.net(pcl, covs)
        loss = segmentation_loss(pred, gt) if hist is None else point_loss(pred, hist)
        loss.backward()
        tr.opt.step()
        acc = accuracy_tensor(pred.detach(), gt) if hist is None else point_accuracy_tensor(pred.detach(), hist)
        return loss.detach(), acc

    def __call__(self, points: torch.Tensor, gt_points: torch.Tensor,
                 counts=None) -> Tuple[torch.Tensor, torch.Tensor]:
        return _replay_step(self, points, gt_points, counts)


class _BaselineBuffers:
    """Every intermediate of the baseline step's front -- sampler, rows,
    histogram -- for one batch shape, allocated once (the captured step)."""

    def __init__(self, B: int, n: int, S: int, cols: int, device, sampler: str, loss: str) -> None:
        i32 = dict(dtype=torch.int32, device=device)
        self.samples = torch.empty((B, S, 3), dtype=torch.float32, device=device)
        self.sample_labels = torch.empty((B, S), **i32)
        self.sample_counts = torch.empty((B,), **i32)
        self.indices = torch.empty((B, S), **i32)
        self.min_dist = torch.empty((B, n), dtype=torch.float32, device=device) if sampler == "fps" else None
        self.rows = torch.empty((B, n), **i32) if loss == "points" else None
        self.hist = torch.empty((B, S, cols), **i32)


class BaselineTrainer:
    """The PointNet baseline's training step: one ``PointNetSegmentation`` +
    Adam (+ DDP when a process group is active), on whole (ragged) scans.

    A training step is: the trainer's ``Augment``, if it has one (its device
    counts feed the sampler) -> the sampler -> the train-mode forward on the
    HIP train blocks -> the loss on integer labels -> backward -> Adam.

    ``sampler="random"`` (the reference's ``np.random.choice`` cut, on the
    GPU): a ``RandomSample(n_samples, seed)`` the trainer owns
    (``self.random_sample``).  ``sampler="fps"``: ``farthest_point_sample``
    and ``gather_samples`` -- what the evaluation samples with, at some 30
    times the cost of the rest of the step at 16 x 100k.

    ``loss="samples"`` (the reference's objective): every existing sample is
    scored against its own label -- ``point_loss`` on the histogram of the
    sample labels over the rows ``0 .. S - 1``; the filler rows of a short
    cloud carry label -1 and no weight.  ``loss="points"`` (what
    ``segment.segment_points_fps`` is scored by): every point of the
    (augmented) scan is scored under its nearest sample
    (``nearest_sample`` -> ``row_histogram`` -> ``point_loss``), exactly the
    mean NLL of what the evaluation would predict for every labelled point.
    A label equal to ``ignore_label`` or outside ``0 .. num_classes`` carries
    no weight under either.

    ``step``, ``step_graphed``, ``graph_inputs`` and ``set_epoch`` are
    ``Trainer``'s: labels one-hot ``[B, n, C + 1]`` or integer ids ``[B, n]``,
    ``counts`` for a ragged batch, ``graphs=True`` (one GPU, no DDP) replays
    the whole step as one HIP graph with the learning rate in a device tensor.
    A trainer captures ONE step: the first batch fixes the points' shape, the
    label form and whether counts come with it, and a batch of another shape
    is a ``ValueError`` -- pad ragged scans to one length and give ``counts``,
    which one graph serves whatever they are.  (Several captured steps in one
    trainer share its gradients, optimizer state, sampler scratch and
    counters; that is not supported here.)  ``step(train=False)`` never augments, runs the eval
    forward (the HIP chains) and samples with a counter of its own fixed at
    ``2^61`` that never advances: validation is deterministic, leaves the
    training draws alone and updates nothing."""

    SAMPLERS = ("random", "fps")
    LOSSES = ("samples", "points")
    EVAL_STEP = 1 << 61

    def __init__(self, model: torch.nn.Module, lr: float, n_samples: int, num_classes: int,
                 device: torch.device, ddp: Optional[bool] = None, bucket_cap_mb: float = 4.0,
                 graphs: bool = False, sampler: str = "random", loss: str = "samples",
                 ignore_label: int = -1, augment=None, seed: int = 0) -> None:
        if sampler not in self.SAMPLERS:  # (checked before any GPU work)
            raise ValueError(f"sampler must be one of {self.SAMPLERS}, got {sampler!r}")
        if loss not in self.LOSSES:
            raise ValueError(f"loss must be one of {self.LOSSES}, got {loss!r}")
        if augment is not None:
            from .augment import Augment
            if not isinstance(augment, Augment):
                raise ValueError(f"augment must be an ndnet.augment.Augment, got {type(augment).__name__}")
        from .preprocessing.sample import RandomSample
        self.random_sample = RandomSample(n_samples, seed)  # (validates n_samples and seed)
        self.augment = augment
        self.sampler, self.loss, self.ignore_label = sampler, loss, int(ignore_label)
        import torch.distributed as dist
        device = torch.device(device)
        self.model = model.to(device)
        self.device = device
        self.n_samples, self.num_classes = int(n_samples), int(num_classes)
        self.base_lr = float(lr)
        if ddp is None:
            ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if graphs and (ddp or device.type != "cuda"):
            raise ValueError("graphs=True needs one GPU and no DDP (the gradient all-reduce is not captured)")
        self.graphs = bool(graphs)
        self._graphed: dict = {}
        self._iota: dict = {}
        self._eval_step: Optional[torch.Tensor] = None
        if ddp:
            from torch.nn.parallel import DistributedDataParallel as DDP
            ids = [device.index if device.index is not None else torch.cuda.current_device()] \
                if device.type == "cuda" else None
            self.net = DDP(self.model, device_ids=ids, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True)
        else:
            self.net = self.model
        if self.graphs:
            self.opt = HipAdam(self.model.parameters(), lr=torch.tensor(self.base_lr, device=device))
        else:
            self.opt = torch.optim.Adam(self.model.parameters(), lr=self.base_lr)
        self.random_sample.resolve_stream()  # (after the DDP set-up: the rank by default)
        if augment is not None:
            augment.resolve_stream()

    set_epoch = Trainer.set_epoch

    def _rows_iota(self, B: int) -> torch.Tensor:
        """Row t of every cloud is sample t: the rows of ``loss="samples"``."""
        r = self._iota.get(B)
        if r is None:
            r = self._iota[B] = torch.arange(self.n_samples, dtype=torch.int32, device=self.device).repeat(B, 1)
        return r

    def samples_and_targets(self, points: torch.Tensor, gt_points: torch.Tensor, counts=None, *,
                            train: bool = True, buffers: Optional[_BaselineBuffers] = None):
        """The front of a step, all on the GPU: ``(samples [B, S, 3], hist
        [B, S, C + 1] int32, sample_counts [B] int32)``.  ``train=True`` puts
        the trainer's ``Augment`` in front and advances the sampler's counter;
        ``train=False`` draws from the eval counter and leaves it.  The eager
        and the captured step both run this."""
        from . import segment
        from .preprocessing.ndtnet_preprocessing import check_class_ids, check_counts, class_ids
        from .preprocessing.sample import gather_samples
        check_class_ids(gt_points, points)
        if points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError(f"points must be [B, n, 3], got {tuple(points.shape)}")
        B, n, _ = points.shape
        S, dev, buf = self.n_samples, self.device, buffers
        if S > n:
            raise ValueError(f"n_samples = {S} needs scans padded to at least that many points, got n = {n}")
        if counts is not None:
            check_counts(counts, B, n)
            counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
        pts = points.to(device=dev, dtype=torch.float32).contiguous()
        labels = class_ids(gt_points, dev)  # ids as they come, or ndnet_row_argmax of a one-hot
        if train and self.augment is not None:
            pts, labels, kept = self.augment(pts, labels, counts)
            if counts is not None or self.augment.drop > 0:
                counts = kept
        out = {} if buf is None else dict(out_points=buf.samples, out_labels=buf.sample_labels,
                                          out_counts=buf.sample_counts)
        if self.sampler == "random":
            if not train and self._eval_step is None:
                self._eval_step = torch.tensor([self.EVAL_STEP], dtype=torch.int64, device=dev)
            smp, slab, scnt, _ = self.random_sample(
                pts, labels, counts, advance=train, step=None if train else self._eval_step,
                out_indices=None if buf is None else buf.indices, **out)
        else:
            from .preprocessing.fps import farthest_point_sample
            idx = farthest_point_sample(pts, S, counts=counts, out=None if buf is None else buf.indices,
                                        min_dist=None if buf is None else buf.min_dist)
            smp, slab, scnt = gather_samples(pts, idx, labels, **out)
        cols = self.num_classes + 1
        hist_out = None if buf is None else buf.hist
        if self.loss == "samples":
            hist = segment.row_histogram(self._rows_iota(B), slab, S, cols, self.ignore_label, out=hist_out)
        else:
            from .preprocessing.nearest import nearest_sample
            rows = nearest_sample(pts, smp, counts=counts, sample_counts=scnt, out=None if buf is None else buf.rows)
            hist = segment.row_histogram(rows, labels, S, cols, self.ignore_label, out=hist_out)
        return smp, hist, scnt

    def step_on_samples(self, samples: torch.Tensor, hist: torch.Tensor, train: bool = True) -> Tuple[float, float]:
        """Forward (+ backward + Adam step when ``train``) on sampled points
        ``[B, S, 3]`` and the rows' class histograms ``[B, S, C + 1]``."""
        if train:
            self.model.train()
            pred = self.net(samples)
            loss = point_loss(pred, hist)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            self.opt.step()
        else:
            self.model.eval()
            with torch.no_grad():
                pred = self.model(samples)
                loss = point_loss(pred, hist)
        return loss.item(), point_accuracy_tensor(pred.detach(), hist).item()

    def step(self, points: torch.Tensor, gt_points: torch.Tensor, train: bool = True,
             counts=None) -> Tuple[float, float]:
        """One batch of whole scans: ``points`` [B,n,3], ``gt_points`` one-hot
        [B,n,C+1] or integer class ids [B,n], ``counts`` the per-cloud point
        counts of a ragged batch -> ``(loss, accuracy)``."""
        if train and self.graphs:
            loss, acc = self.step_graphed(points, gt_points, counts)
            return loss.item(), acc.item()
        smp, hist, _ = self.samples_and_targets(points, gt_points, counts, train=train)
        return self.step_on_samples(smp, hist, train)

    def _graph_for(self, points_shape, gt_shape, ragged: bool = False) -> "GraphedBaselineStep":
        key = (tuple(points_shape), tuple(gt_shape)) + ((True,) if ragged else ())
        g = self._graphed.get(key)
        if g is None:
            if self._graphed:  # one captured step per trainer: see the class docstring
                have = next(iter(self._graphed))
                raise ValueError(f"BaselineTrainer(graphs=True) captures one batch shape and has captured {have}; "
                                 f"got {key}.  Pad the batches to one length (counts say where a cloud ends) and "
                                 "keep one label form and the choice of counts, or use graphs=False")
            gt_width = gt_shape[-1] if len(gt_shape) == 3 else None  # None: integer class ids
            g = self._graphed[key] = GraphedBaselineStep(self, points_shape, gt_width, ragged=ragged)
        return g

    def step_graphed(self, points: torch.Tensor, gt_points: torch.Tensor,
                     counts=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """A training step as a graph replay; returns (loss, accuracy) as device
        scalars, without synchronising (``Trainer.step_graphed``)."""
        from .preprocessing.ndtnet_preprocessing import check_class_ids, check_counts
        check_class_ids(gt_points, points)
        if counts is not None:
            check_counts(counts, points.shape[0], points.shape[1])
        return self._graph_for(points.shape, gt_points.shape, counts is not None)(points, gt_points, counts)

    def graph_inputs(self, points_shape, gt_shape, counts: bool = False):
        """The static (points, gt[, counts]) buffers the captured step of this
        shape reads (``Trainer.graph_inputs``)."""
        g = self._graph_for(points_shape, gt_shape, bool(counts))
        return (g.s_points, g.s_gt, g.s_counts) if counts else (g.s_points, g.s_gt)


class GraphedBaselineStep:
    """The baseline's training step for one input shape, captured once and
    replayed, built like ``GraphedTrainStep``: static input buffers
    (``s_points``, ``s_gt`` float one-hot or int32 ids, ``s_counts`` with
    ``ragged=True``) and every sampler / rows / histogram buffer allocated
    once; a few eager steps on a side stream first; parameters, buffers,
    optimizer state, the sampler's counter and the augmentation's snapshotted
    before them and restored after the capture, so the first replay is draw 0
    of the trainer's first step and every replay draws anew."""

    def __init__(self, trainer: BaselineTrainer, points_shape, gt_width: Optional[int], warmup: int = 3,
                 ragged: bool = False) -> None:
        tr = self.tr = trainer
        dev = tr.device
        B, n = int(points_shape[0]), int(points_shape[1])
        if tr.n_samples > n:
            raise ValueError(f"n_samples = {tr.n_samples} needs scans padded to at least that many points, got n = {n}")
        self.s_points = torch.zeros((B, n, 3), dtype=torch.float32, device=dev)
        if gt_width is None:  # integer class ids (class 0 for the warm-up steps)
            self.s_gt = torch.zeros((B, n), dtype=torch.int32, device=dev)
        else:
            self.s_gt = torch.zeros((B, n, int(gt_width)), dtype=torch.float32, device=dev)
            self.s_gt[..., 0] = 1.0
        self.s_counts = torch.full((B,), n, dtype=torch.int32, device=dev) if ragged else None
        self.buffers = _BaselineBuffers(B, n, tr.n_samples, tr.num_classes + 1, dev, tr.sampler, tr.loss)
        gen = torch.Generator(device=dev).manual_seed(0)
        self.s_points.copy_(torch.rand(self.s_points.shape, device=dev, generator=gen) * 20 - 10)
        counters = [tr.random_sample.step_tensor(dev)]
        if tr.augment is not None:
            counters.append(tr.augment.step_tensor(dev))
        self.graph, (self.loss, self.acc) = _capture_step(tr.model, tr.opt, dev, self._body, counters, warmup)

    def _body(self):
        tr = self.tr
        smp, hist, _ = tr.samples_and_targets(self.s_points, self.s_gt, self.s_counts, train=True,
                                              buffers=self.buffers)
        tr.model.train()
        pred = tr.net(smp)
        loss = point_loss(pred, hist)
        loss.backward()
        tr.opt.step()
        return loss.detach(), point_accuracy_tensor(pred.detach(), hist)

    def __call__(self, points: torch.Tensor, gt_points: torch.Tensor,
                 counts=None) -> Tuple[torch.Tensor, torch.Tensor]:
        return _replay_step(self, points, gt_points, counts)
