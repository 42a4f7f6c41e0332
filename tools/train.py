#!/usr/bin/env python3
"""Counterpart of the reference's tools/train.py (segmentation task) on the
HIP path, one process per GPU:

    python tools/train.py --epochs 2 --steps-per-epoch 4
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
        tools/train.py --epochs 2                      # DDP over RCCL

The CARLA PLY dataset (ndnet/datasets/CARLA_Seg.py) is not available here,
so batches are labelled synthetic L clouds (ndnet.synthetic), a different
seed per rank and step.  Arguments keep the reference's names and defaults
(train.py:97-111) where they apply; the step itself is ndnet.training.Trainer
(its docstring lists the reference defects fixed on the way).  Checkpoints are
saved under the reference's file names (train.py:191-193).

``--model pointnet`` trains the PointNet baseline instead (the reference's
tools/train_pointnet.py) with ndnet.training.BaselineTrainer: whole scans --
ragged from disk (``collate_padded``) or synthetic -- cut to ``--n_samples``
points on the GPU by ``--sampler`` inside the step.  ``--graphs`` goes with the
synthetic scans only: the baseline's captured step takes one batch shape, and
scans from disk come padded to each batch's own longest.

    python tools/train.py --model pointnet --n_samples 4160 --graphs --epochs 2
"""
import argparse
import datetime
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))

from ndnet import distributed as D  # noqa: E402
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.synthetic import make_labelled_batch  # noqa: E402
from ndnet.training import BaselineTrainer, Trainer  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="segmentation")
    ap.add_argument("--n_desired_nds", type=int, default=2080)
    ap.add_argument("--n_samples", type=int, default=70000)
    ap.add_argument("--out_path", default="out")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--save_every", type=int, default=2)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--learning_rate", type=float, default=0.034)
    ap.add_argument("--n_classes", type=int, default=28)
    ap.add_argument("--feature_dim", type=int, default=768)
    ap.add_argument("--train_path", default=None, help="CARLA PLY scans (ndnet.datasets.CARLA_Seg); synthetic if absent")
    ap.add_argument("--val_path", default=None)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--steps-per-epoch", type=int, default=8, help="synthetic batches per epoch and rank")
    ap.add_argument("--val-steps", type=int, default=2)
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--graphs", action="store_true",
                    help="one GPU: replay each training step from a captured HIP graph (Trainer(graphs=True))")
    ap.add_argument("--loss", default="nds", choices=["nds", "points"],
                    help="nds: the NLL of each ND's hard class; points: the mean NLL of every labelled point "
                         "under the ND row it was folded into (Trainer(loss=...))")
    ap.add_argument("--point-fill", default="nearest", choices=["nearest", "none"],
                    help="loss=points: the row of a point of a pruned ND")
    ap.add_argument("--ignore-label", type=int, default=-1, help="loss=points: a label left out of the loss")
    ap.add_argument("--augment", action="store_true",
                    help="augment every training batch on the GPU (ndnet.augment.Augment; the rank is its stream)")
    ap.add_argument("--aug-yaw", type=float, default=180.0, help="largest yaw about z, degrees")
    ap.add_argument("--aug-scale", type=float, nargs=2, default=(0.95, 1.05), metavar=("LO", "HI"))
    ap.add_argument("--aug-flip", type=float, nargs=2, default=(0.0, 0.5), metavar=("PX", "PY"),
                    help="probabilities of mirroring x and y")
    ap.add_argument("--aug-shift", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("SX", "SY", "SZ"))
    ap.add_argument("--aug-jitter", type=float, default=0.0, help="standard deviation of the per-point noise")
    ap.add_argument("--aug-drop", type=float, default=0.0,
                    help="largest share of a cloud's points dropped (each cloud draws its own share below it)")
    ap.add_argument("--aug-seed", type=int, default=0)
    ap.add_argument("--model", default="ndtnet", choices=["ndtnet", "pointnet"],
                    help="pointnet: the baseline on --n_samples points of every whole scan (BaselineTrainer)")
    ap.add_argument("--sampler", default="random", choices=["random", "fps"],
                    help="model=pointnet: how the step cuts a scan to --n_samples points")
    ap.add_argument("--baseline-loss", default="samples", choices=["samples", "points"],
                    help="model=pointnet: every sample against its own label, or every point of the scan under "
                         "its nearest sample (BaselineTrainer(loss=...))")
    ap.add_argument("--scan-points", type=int, default=100_000, help="model=pointnet: points of a synthetic scan")
    ap.add_argument("--sample-seed", type=int, default=0, help="model=pointnet: the random sampler's seed")
    args = ap.parse_args()
    if args.model == "pointnet" and args.graphs and args.train_path:
        raise SystemExit("--model pointnet --graphs runs on synthetic scans only: BaselineTrainer(graphs=True) "
                         "captures one batch shape, and collate_padded pads every batch of whole scans to its own "
                         "longest scan; run without --graphs")
    if args.task != "segmentation":
        raise NotImplementedError("only the segmentation task is on the hot path (train.py:122-123)")

    rank, local, world = D.world_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    D.init("nccl", dev)
    torch.manual_seed(0)  # identical initial weights on every rank (DDP also broadcasts rank 0's)
    baseline = args.model == "pointnet"
    if baseline:
        from ndnet.models.pointnet import PointNetSegmentation
        model = PointNetSegmentation(3, args.n_classes, args.feature_dim)
    else:
        model = NDTNetSegmentation(3, args.n_classes, args.feature_dim)
    if args.graphs and world > 1:
        raise SystemExit("--graphs runs on one GPU (the DDP all-reduce is not captured)")
    augment = None
    if args.augment:
        import math
        from ndnet.augment import Augment
        augment = Augment(yaw=math.radians(args.aug_yaw), scale=tuple(args.aug_scale), flip=tuple(args.aug_flip),
                          shift=tuple(args.aug_shift), jitter=args.aug_jitter, drop=args.aug_drop, seed=args.aug_seed)
    if baseline:
        tr = BaselineTrainer(model, args.learning_rate, args.n_samples, args.n_classes, dev, graphs=args.graphs,
                             sampler=args.sampler, loss=args.baseline_loss, ignore_label=args.ignore_label,
                             augment=augment, seed=args.sample_seed)
    else:
        tr = Trainer(model, args.learning_rate, args.n_desired_nds, args.n_classes, dev, graphs=args.graphs,
                     loss=args.loss, point_fill=args.point_fill, ignore_label=args.ignore_label, augment=augment)
    path = os.path.join(args.out_path, datetime.datetime.now().strftime("%Y%m%d_%H%M%S"))

    loaders = {}
    if args.train_path:
        from ndnet.datasets.carla_seg import CARLA_Seg, collate_padded, loader
        from torch.utils.data.distributed import DistributedSampler
        for mode, pth in (("train", args.train_path), ("val", args.val_path or args.train_path)):
            # the baseline takes whole scans, padded to the batch's longest, and cuts them on the GPU
            ds = CARLA_Seg(args.n_classes, None if baseline else args.n_samples, pth)
            collate = dict(collate_fn=collate_padded) if baseline else {}
            sampler = DistributedSampler(ds, world, rank) if world > 1 else None
            loaders[mode] = torch.utils.data.DataLoader(
                ds, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler, pin_memory=True,
                num_workers=args.num_workers, drop_last=True, **collate) if world > 1 else loader(
                    ds, args.batch_size, num_workers=args.num_workers, **collate)

    def batches(epoch: int, mode: str, steps: int):
        if mode in loaders:  # scans from disk, parsed ahead by the loader's workers
            for pcl, gt, *counts in loaders[mode]:  # (collate_padded adds the counts)
                if pcl.shape[0] > 1:  # train.py:49-51 skips single-cloud batches
                    yield pcl.to(dev, non_blocking=True), gt.to(dev, non_blocking=True), (counts[0] if counts else None)
            return
        n = args.scan_points if baseline else args.n_samples
        for s in range(steps):
            seed = ((epoch * 1000 + s) * world + rank) * args.batch_size + (0 if mode == "train" else 10 ** 7)
            pts, gt = make_labelled_batch(args.batch_size, n, args.n_classes, seed0=seed)
            if baseline:  # integer ids: the baseline needs no one-hot
                yield torch.from_numpy(pts), torch.from_numpy(gt.argmax(-1).astype("int32")), None
            else:
                yield torch.from_numpy(pts), torch.from_numpy(gt), None

    def run(epoch: int, mode: str, steps: int):
        tot_loss = tot_acc = 0.0
        t0 = time.perf_counter()
        s = -1
        for s, (pts, gt, counts) in enumerate(batches(epoch, mode, steps)):
            if counts is None:
                loss, acc = tr.step(pts, gt, train=mode == "train")
            else:
                loss, acc = tr.step(pts, gt, train=mode == "train", counts=counts)
            tot_loss += loss
            tot_acc += acc
            if rank == 0:
                print(f"{mode} epoch {epoch + 1} step {s + 1}/{steps}: loss {loss:.4f} acc {acc:.3f}", flush=True)
        torch.cuda.synchronize()
        dt = D.max_over_ranks(time.perf_counter() - t0)
        n = max(s + 1, 1)
        return tot_loss / n, tot_acc / n, dt, n

    for epoch in range(args.epochs):
        tr.set_epoch(epoch)
        for ld in loaders.values():
            if isinstance(getattr(ld, "sampler", None), torch.utils.data.distributed.DistributedSampler):
                ld.sampler.set_epoch(epoch)
        loss, acc, dt, nb = run(epoch, "train", args.steps_per_epoch)
        if rank == 0:
            print(f"--- epoch {epoch + 1}/{args.epochs}: train loss {loss:.4f} acc {acc:.3f}, "
                  f"{world * args.batch_size * nb / dt:.1f} clouds/s over {world} rank(s)")
        vloss, vacc, _, _ = run(epoch, "val", args.val_steps)
        if rank == 0:
            print(f"--- epoch {epoch + 1}: val loss {vloss:.4f} acc {vacc:.3f}")
        if rank == 0 and not args.no_save and (epoch + 1) % args.save_every == 0:
            os.makedirs(path, exist_ok=True)
            torch.save(model.state_dict(), f"{path}/{args.model}_{args.task}_full_{epoch + 1}.pth")
            torch.save(model.feature_extractor.state_dict(), f"{path}/{args.model}_{args.task}_backbone_{epoch + 1}.pth")
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
