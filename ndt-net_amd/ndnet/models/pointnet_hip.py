"""Eval-mode NDTNetSegmentation forward on the HIP point-MLP kernel.

The reference forward (ndnet/models/ndtnet.py:112-164, 218-243) is rewritten
as four fused point-MLP chains (``ndnet_pn_chain_run``, csrc/pointnet_kernels.hip)
with small per-cloud steps between them:

  A  TNet(3):   p -> 64 -> 128 -> 1024, max over points          -> g1
     FC head (1024 -> 512 -> 256 -> 9) + I                       -> t1
  B  conv1 with t1 folded in (x' = [t1 p, t1 C] is linear in x), then
     TNet(64):  -> 64 -> 64 -> 128 -> 1024, max                  -> g2
     FC head (1024 -> 512 -> 256 -> 4096) + I                    -> t2
  C  conv2 with t2^T folded in (x_t2 = t2^T x1), conv3, max      -> g3 [F]
     (no ReLU in it: in the x6 / fp32 modes one per-cloud 12 -> F layer,
     ``ndnet_pn_pool12_run``, in the chain's place; ``BACKBONE``; by default
     from the fold's composed tail W2'^T W3'^T, ``ndnet_pn_pool12_tail_run``;
     ``FOLD_PRODUCTS``)
  D  seg conv1 split: W[:, :64] t2^T x1 per point + (W[:, 64:] g3 + b) per
     cloud (the reference concatenates the broadcast g3 to every point:
     ndtnet.py:227-230), -> 512 -> 256 -> 128 -> C+1, log_softmax

In the x6 mode chains B and D each run one layer fewer (``COLLAPSE``): nothing
non-linear separates conv1 from TNet(64)'s first layer or from the seg head's
conv1 on the point features, so B's layer 0 is the per-cloud 12 -> 64 layer
relu(x (W1f[b] M) + (b1 M + bM)), composed in its prologue, and D opens with a
per-cloud 12 -> 512 layer (``ndnet_pn_fold_seg_run`` writes its weights,
``ndnet_pn_fc_mfma_bias_run`` its bias rows) fused into 512 -> 256.

In that default forward (the composed tail, B and D collapsed) the split layers of chains A, B and
D run on two fp16 slices and three products instead of three bf16 slices and six (``SLICES``,
``ndnet_pn_chain_f16_run``): the same accuracy class on half the matrix instructions, each tile
falling back to the bf16 code inside the launch when its activations leave fp16's window.

Every BatchNorm (running statistics) is folded into the preceding 1x1 conv /
linear layer.  The per-point GEMMs run on the matrix cores: eleven layers
(the three 128 -> 1024 / F max-pooled convs, the t2-folded conv2, the seg
head's 64 -> 512, 512 -> 256, 256 -> 128 and 128 -> C+1, and the TNets'
64 -> 64 / 64 -> 128; ``X6_NARROW``) as fp32-accurate split-bf16 products
(``SPLIT_BF16`` below), the K = 16 first layers on the fp32 MFMA.  The
per-cloud steps (TNet FC heads and the seg head's global-feature bias on the
fp32 MFMA, ``ndnet_pn_fc_mfma_run``; the t1 / t2 weight folds) are HIP
kernels on the same stream (``_glue_hip``); ``_glue_torch`` is their torch
restatement for the tests.

NDTNetClassification (``classification_forward``) shares chains A-C, the
per-cloud steps, the fold and the workspace; instead of D its head
(ndtnet.py:188-194, no BatchNorm) runs on the pooled g3 per cloud:
relu(conv1: F -> 512) and relu(conv2: 512 -> 256) as two
``ndnet_pn_fc_mfma_run`` launches, then conv3 (256 -> num_classes) and the
softmax in one ``ndnet_pn_cls_head_run``, which also re-arms the max-pool
buffer -> probabilities [B, num_classes, 1].

The PointNet-on-FPS baseline (``ndnet.models.pointnet``; ``_Folded.baseline``)
runs the same chains on [B, N, 3] points.  The reference clamps the transformed
points, nan_to_num(t1 p), which is not linear, so t1 is not folded into conv1:
chain A reads the points, fc3 (GEMV) gives t1, ``ndnet_pn_transform3_run``
(include/ndnet_nearest.h) writes the transformed points, chain B's layer 0 is
the shared conv1, and chain C folds t2 through it in its prologue and
publishes the result for chain D.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

from .. import _lib

MAX_LAYERS = 5
CHAIN_NAMES = ("A: TNet(3) 3-64-128-1024 + max", "B: conv1(t1) + TNet(64) 64-64-128-1024 + max",
               "C: conv1, conv2(t2), conv3 + max", "D: seg head 64-512-256-128-(C+1) + log_softmax")

# set to a list to collect (chain index, start event, end event) per chain launch
chain_timing = None

# The three wide max-pooled layers (TNet(3) / TNet(64) conv3, NDTNet conv3:
# 128 -> 1024 / 768, 90% of chains A-C's FLOPs) and the seg head's 512 -> 256
# (fed chunk by chunk from the fused 64 -> 512), the 64 -> 512 itself, 256 -> 128
# and NDTNet's t2-folded conv2 run as split-bf16 "x6" GEMMs
# (include/ndnet_pointnet.h prec = 1): fp32-accurate (operands split into
# three bf16, six exact partial products accumulated in fp32) on the bf16
# matrix cores.  NDNET_PN_PRECISION: "x6" (default), "fp32" to keep every
# layer on the fp32 MFMA, or one of the reduced modes of the same layers, which
# trade accuracy for matrix-core work on the same folded weights (prec 2 / 3):
#   "x3"    three products (h h' + h m' + m h'): 16 significant bits per operand,
#           dropped terms <= 3.02 * 2^-18 |a w| per product
#   "bf16"  one product (h h'): plain bf16 operands, fp32 accumulation,
#           dropped terms <= (2^-8 + 2^-18) |a w| -- autocast level
# Measured errors and times: DESIGN.md, the section on the split-bf16 layers.
# (Round 2's "x6f" -- fp32 weights split in registers, measured 20-25% slower
# per layer -- was removed in round 3: its code paths alone cost the kernel
# registers and scratch, profiles/r03l_stamps_depth.txt.  The reduced modes are
# whole-kernel instantiations of their own and leave x6's code as it was.)
MODES = {"x6": 1, "fp32": 1, "x3": 2, "bf16": 3}  # mode -> ndnet_pn_layer.prec of the split layers
PRECISION = SPLIT_BF16 = X6_PREC = None


def set_precision(mode: str) -> None:
    """The module-wide mode, "x6", "x3", "bf16" or "fp32": what every model
    whose ``precision`` attribute is None runs from its next forward on (the
    folded weights serve every mode; argument blocks are kept per mode)."""
    global PRECISION, SPLIT_BF16, X6_PREC
    if mode not in MODES:
        raise ValueError(f"unknown PointNet precision mode {mode!r}")
    PRECISION = mode
    SPLIT_BF16 = mode != "fp32"
    X6_PREC = MODES[mode]


def model_precision(model) -> str:
    """The mode ``model``'s next forward runs: its ``precision`` attribute, or
    the module-wide mode when that is None."""
    mode = getattr(model, "precision", None)
    if mode is None:
        return PRECISION
    if mode not in MODES:
        raise ValueError(f"unknown PointNet precision mode {mode!r}")
    return mode


set_precision(os.environ.get("NDNET_PN_PRECISION", "x6"))
# split-bf16 also on the narrower per-point layers with K >= 64 (TNet(3)'s
# 64 -> 128, TNet(64)'s 64 -> 64 and 64 -> 128, the seg head's 128 -> C+1):
# default on, measured -5 us per forward (chains A / B / D 3 / 2 / 1.5 us
# faster); "0" keeps them on the fp32 MFMA.  Only the K = 16 first layers stay fp32.
X6_NARROW = os.environ.get("NDNET_PN_X6_NARROW", "1") == "1"


# Model widths the eval kernels take (``supports``).  feature_dim: the seg
# head's global-feature bias is one ndnet_pn_fc_mfma_run with K = F (<= 1024),
# and the 32-point chain build stages a layer's bias two values per thread
# (N <= 1024); any F up to that runs (padded to 16 / 64 columns with zeros).
# num_classes: chain D's logits are fp32 rows of LDS region 1 beside its
# 256-wide bf16 planes; 64 points x 448 columns is what the 64-point build's
# 160 KB hold.  A model outside these runs ndtnet's torch composition.
MAX_FEATURE_DIM = 1024
MAX_LAST_N = 448
MAX_CLASSES = 1024  # NDTNetClassification: ndnet_pn_cls_head_run's padded N
X6_LAST_MAX_N = 64  # 128 -> C+1 as a split-bf16 layer up to this padded width (_Folded)
COLLAPSE_D_MAX_LAST_N = 256  # chain D opens with the collapsed 12 -> 512 layer up to this padded width (collapses_d)


def supports_classification(model) -> bool:
    """The same for an ``NDTNetClassification``: its head's conv1 is one
    ndnet_pn_fc_mfma_run with K = F (<= 1024), and ndnet_pn_cls_head_run keeps
    a 16-cloud chunk's logits in LDS (16 x 1024 floats: num_classes <= 1024)."""
    F = model.feature_dim
    return (1 <= F <= MAX_FEATURE_DIM and (FC_MFMA or F % 4 == 0) and 1 <= model.num_classes <= MAX_CLASSES
            and model.point_dim == 3)


def supports(model) -> bool:
    """Whether the eval kernels take this model's widths; if not, the model's
    forward runs the torch composition (``forward_torch``) instead."""
    F, C1 = model.feature_dim, model.num_classes + 1
    return (1 <= F <= MAX_FEATURE_DIM and (FC_MFMA or F % 4 == 0)  # the GEMV kernel reads 16-byte pieces
            and _npad(C1) <= MAX_LAST_N)


class _Layer(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("w_cloud_stride", ctypes.c_int64), ("bias", ctypes.c_void_p),
                ("bias_cloud_stride", ctypes.c_int64), ("K", ctypes.c_int32), ("N", ctypes.c_int32),
                ("relu", ctypes.c_int32), ("prec", ctypes.c_int32), ("fuse_next", ctypes.c_int32)]


class _Chain(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("x_ld", ctypes.c_int32), ("in_cols", ctypes.c_int32),
                ("num_points", ctypes.c_int32), ("num_layers", ctypes.c_int32), ("L", _Layer * MAX_LAYERS),
                ("mode", ctypes.c_int32), ("out_cols", ctypes.c_int32), ("gmax", ctypes.c_void_p),
                ("gmax_ld", ctypes.c_int32), ("max_width", ctypes.c_int32), ("max_width2", ctypes.c_int32),
                ("out", ctypes.c_void_p), ("clear", ctypes.c_void_p), ("clear_count", ctypes.c_int64),
                ("head_h2", ctypes.c_void_p), ("head_ld", ctypes.c_int32), ("head_K", ctypes.c_int32),
                ("head_w3", ctypes.c_void_p), ("head_b3", ctypes.c_void_p), ("head_basis", ctypes.c_void_p),
                ("head_kin", ctypes.c_int32), ("head_nout", ctypes.c_int32), ("head_t1", ctypes.c_void_p),
                ("fold_t2", ctypes.c_void_p), ("fold_ld", ctypes.c_int32), ("fold_out_w", ctypes.c_void_p),
                ("fold_out_b", ctypes.c_void_p), ("fold_bias", ctypes.c_void_p),
                ("x_nonfinite_nan", ctypes.c_int32), ("reserved0", ctypes.c_int32)]


class _F16(ctypes.Structure):  # ndnet_pn_f16: what the fp16 two-slice form adds to a chain's argument block
    _fields_ = [("w16", ctypes.c_void_p * MAX_LAYERS), ("scale", ctypes.c_void_p * MAX_LAYERS),
                ("fallbacks", ctypes.c_void_p)]


class _Fold16Job(ctypes.Structure):  # ndnet_pn_fold16_job
    _fields_ = [("w", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("var", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("partial", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("N", ctypes.c_int32), ("K", ctypes.c_int32), ("ld", ctypes.c_int32), ("k0", ctypes.c_int32),
                ("Kp", ctypes.c_int32), ("Np", ctypes.c_int32), ("eps", ctypes.c_float),
                ("reserved", ctypes.c_int32)]


class _FoldJob(ctypes.Structure):  # ndnet_pn_fold_job (include/ndnet_pointnet.h)
    _fields_ = [("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p),
                ("beta", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("var", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("kind", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
                ("ld", ctypes.c_int32), ("k0", ctypes.c_int32), ("Kp", ctypes.c_int32), ("Np", ctypes.c_int32),
                ("eye", ctypes.c_int32), ("eps", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("block0", ctypes.c_int64), ("rhs", ctypes.c_void_p), ("out_f64", ctypes.c_int32),
                ("reserved1", ctypes.c_int32)]



def available() -> bool:
    try:
        return torch.cuda.is_available() and hasattr(_lib.lib(), "ndnet_pn_chain_run")
    except RuntimeError:
        return False


def _pad(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _bn_fold(w: torch.Tensor, b: torch.Tensor, bn: torch.nn.BatchNorm1d):
    """y = bn(W x + b) -> W' x + b' (eval statistics)."""
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return w * s[:, None], (b - bn.running_mean) * s + bn.bias


def _wT(w: torch.Tensor, kpad: int, npad: int) -> torch.Tensor:
    """[N][K] weight -> zero-padded transposed [Kpad][Npad] fp32, contiguous."""
    n, k = w.shape
    out = torch.zeros((kpad, npad), dtype=torch.float32, device=w.device)
    out[:k, :n] = w.t()
    return out


def _frag(wT: torch.Tensor) -> torch.Tensor:
    """Plain W^T [..., K, N] (K % 16 == 0, N % 16 == 0) -> the fragment-major
    layout of include/ndnet_pointnet.h, flattened: [cb][kg][kq][cl][s] with
    k = 16 kg + 4 kq + s, n = 16 cb + cl."""
    *lead, K, N = wT.shape
    v = wT.reshape(*lead, K // 16, 4, 4, N // 16, 16)
    nl = len(lead)
    perm = list(range(nl)) + [nl + 3, nl + 0, nl + 1, nl + 4, nl + 2]
    return v.permute(*perm).reshape(*lead, K * N).contiguous()


def _npad(n: int) -> int:
    """Output width the chain kernel splits evenly: 32, or a multiple of 64."""
    return 32 if n <= 32 else _pad(n, 64)


def _frag_x6(wT: torch.Tensor) -> torch.Tensor:
    """Plain W^T [K, N] (K % 32 == 0, N % 16 == 0) -> the split-bf16 layout of
    include/ndnet_pointnet.h (prec 1), flattened bf16: W^T = h + m + l
    (h = bf16(w), m = bf16(w - h), l = bf16(w - h - m), residuals exact in
    fp32), [cb][kg][plane][kq][cl][j] with k = 32 kg + 8 kq + j, n = 16 cb + cl."""
    K, N = wT.shape
    w = wT.float()
    h = w.to(torch.bfloat16)
    r = w - h.float()
    m = r.to(torch.bfloat16)
    lo = (r - m.float()).to(torch.bfloat16)
    planes = torch.stack([h, m, lo])                                  # [3, K, N]
    v = planes.reshape(3, K // 32, 4, 8, N // 16, 16)                 # plane, kg, kq, j, cb, cl
    return v.permute(4, 1, 0, 2, 5, 3).reshape(-1).contiguous()        # cb, kg, plane, kq, cl, j


def _f16_exponent(wmax: float) -> int:
    """The layer-wide exponent s of the fp16 form: max |w| 2^s in [2^13, 2^14), at most 100 (a
    maximum below 2^-87 stays under 2^13; every finite one lands below 2^14: s >= -114, which fp32
    holds); 0 for a maximum that is zero or not finite (ndnet_pn_fold16_run's rule)."""
    if not (wmax > 0.0) or not math.isfinite(wmax):
        return 0
    return min(100, 13 - (math.frexp(wmax)[1] - 1))


def _frag_f16(wT: torch.Tensor):
    """Plain W^T [K, N] (K % 32 == 0, N % 16 == 0) -> (planes, scale): the two fp16 planes of
    ndnet_pn_f16.w16, flattened, and the one float 2^-s the kernel reads with them.  W^T 2^s = h + l with
    h = fp16(w 2^s), l = fp16(w 2^s - h), both to nearest even (the power of two scales exactly),
    [cb][kg][plane][kq][cl][j] with k = 32 kg + 8 kq + j, n = 16 cb + cl: the layout of ``_frag_x6`` with
    two planes per k-group.  Bit for bit what ndnet_pn_fold16_run writes."""
    K, N = wT.shape
    w = wT.float()
    # the device maximum is an fmaxf chain: a NaN weight takes no part in it
    s = _f16_exponent(float(w.abs().nan_to_num(nan=0.0, posinf=float("inf")).max()) if w.numel() else 0.0)
    x = w * (2.0 ** s)
    h = x.to(torch.float16)
    lo = (x - h.float()).to(torch.float16)
    planes = torch.stack([h, lo])                                      # [2, K, N]
    v = planes.reshape(2, K // 32, 4, 8, N // 16, 16)                  # plane, kg, kq, j, cb, cl
    scale = torch.full((1,), 2.0 ** -s, dtype=torch.float32, device=wT.device)
    return v.permute(4, 1, 0, 2, 5, 3).reshape(-1).contiguous(), scale  # cb, kg, plane, kq, cl, j


def _prod64(a: torch.Tensor, rhs: torch.Tensor, bias=None) -> torch.Tensor:
    """a @ rhs (+ bias on every row) as an NDNET_FOLD_PROD job forms it, bit for bit: fp32 factors, each
    product exact in float64, the sum in float64 with k ascending, the bias last."""
    a, rhs = a.reshape(-1, a.shape[-1]).double(), rhs.double()
    acc = torch.zeros((a.shape[0], rhs.shape[1]), dtype=torch.float64, device=a.device)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * rhs[k]
    return acc if bias is None else acc + bias.double()


def _bpad(b: torch.Tensor, npad: int) -> torch.Tensor:
    out = torch.zeros(npad, dtype=torch.float32, device=b.device)
    out[: b.shape[0]] = b
    return out


class _Folded:
    """BN-folded, transposed, padded weights of one model (on its device)."""

    def __init__(self, m) -> None:
        fe = m.feature_extractor
        with torch.no_grad():
            def conv(c, bn):
                return _bn_fold(c.weight[:, :, 0].float(), c.bias.float(), bn)

            def tnet(t):
                w1, b1 = conv(t.conv1, t.bn1)
                w2, b2 = conv(t.conv2, t.bn2)
                w3, b3 = conv(t.conv3, t.bn3)
                f1, c1 = _bn_fold(t.fc1.weight.float(), t.fc1.bias.float(), t.bn4)
                f2, c2 = _bn_fold(t.fc2.weight.float(), t.fc2.bias.float(), t.bn5)
                return dict(w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, f1=f1, c1=c1, f2=f2, c2=c2,
                            f3=t.fc3.weight.float(), c3=t.fc3.bias.float())

            self.seg = hasattr(m, "conv4")  # NDTNetSegmentation; else NDTNetClassification (no BatchNorm in its head)
            # the PointNet-on-FPS baseline (models/pointnet.py): points only, conv1 has 3 inputs and
            # stays a shared layer (t1 is applied to the points, ndnet_pn_transform3_run)
            self.baseline = bool(getattr(fe, "points_only", False))
            F = m.feature_dim
            self.F = F
            # ---- the feature extractor (chains A-C), the same for either model ----
            self.t1 = tnet(fe.t1)
            self.t2 = tnet(fe.t2)
            self.c1w, self.c1b = conv(fe.conv1, fe.bn1)   # [64, 12]
            self.c2w, self.c2b = conv(fe.conv2, fe.bn2)   # [128, 64]
            self.c3w, self.c3b = conv(fe.conv3, fe.bn3)   # [F, 128]
            # shared per-point layers, W^T padded
            t1, t2 = self.t1, self.t2
            self.A = [(_wT(t1["w1"], 16, 64), t1["b1"]), (_wT(t1["w2"], 64, 128), t1["b2"]),
                      (_wT(t1["w3"], 128, 1024), t1["b3"])]
            self.B_tail = [(_wT(t2["w1"], 64, 64), t2["b1"]), (_wT(t2["w2"], 64, 128), t2["b2"]),
                           (_wT(t2["w3"], 128, 1024), t2["b3"])]
            self.C_tail = (_wT(self.c3w, 128, _npad(F)), _bpad(self.c3b, _npad(F)))
            self.c1wT = self.c1w.t().contiguous()         # [12, 64]
            # weight-only products of the forward (``FOLD_PRODUCTS``), each (out, left, right, bias row or
            # None) an NDNET_FOLD_PROD job behind ``jobs`` in the device table, so a re-fold recomputes it
            self.products = []
            # x_t2 = t2^T x1 (ndtnet.py:152-157) feeds conv2 and the seg head's
            # conv1a; t2 is folded into chains C / D's layer 0 (their prologue,
            # ndnet_pn_chain.fold_t2), so both layers keep shared weights
            self.C_mid = (_wT(self.c2w, 64, 128), self.c2b)          # conv2 W^T [64, 128]
            if not self.baseline:
                # chain C's composed tail for ndnet_pn_pool12_tail_run, kept in float64:
                # W23 = W2'^T W3'^T (64 x Fp), b23 = b2' W3'^T + b3' (Fp)
                self.W23 = _prod64(self.C_mid[0], self.C_tail[0])
                self.b23 = _prod64(self.c2b[None, :], self.C_tail[0], self.C_tail[1]).reshape(-1)
                self.products += [(self.W23, self.C_mid[0], self.C_tail[0], None),
                                  (self.b23, self.c2b, self.C_tail[0], self.C_tail[1])]
            # conv1 of the t1-transformed input: (W1 M(t1))^T = sum_ac t1[a,c] E_ac^T W1^T,
            # M(t1) = blockdiag(t1, kron(t1, I3)) (p' = t1 p, C' = t1 C)
            dev = self.c1wT.device
            if self.baseline:
                self.t1_basis = None
                self.c1T16 = _wT(self.c1w, 16, 64)        # conv1 W^T, K padded 3 -> 16 with zero rows
            else:
                E = torch.zeros((9, 12, 12), device=dev)
                for a in range(3):
                    for c in range(3):
                        E[3 * a + c, a, c] = 1.0
                        for j in range(3):
                            E[3 * a + c, 3 + 3 * a + j, 3 + 3 * c + j] = 1.0
                self.t1_basis = torch.matmul(E.transpose(1, 2), self.c1wT).reshape(9, 12 * 64).contiguous()
            # the per-point layers with fragment-major copies (the HIP chains) ...
            self.chain_w = [w for w, _ in self.A + self.B_tail + [self.C_mid, self.C_tail]]
            if self.baseline:
                self.chain_w.append(self.c1T16)
            # ... and the wide pooled layers and conv2 in split-bf16 form
            self.wide = [self.A[2][0], self.B_tail[2][0], self.C_tail[0]]
            # the FC layers of the TNet heads, W^T fragment-major for the MFMA GEMV (ndnet_pn_fc_mfma_run)
            self.fcs = [self.t1["f1"], self.t1["f2"], self.t2["f1"], self.t2["f2"], self.t2["f3"]]
            if self.seg:
                self._fold_seg(m, conv)
            else:
                self._fold_cls(m)
            self.wide.append(self.C_mid[0])
            if self.seg:
                self.wide.append(self.s1aT)
            if X6_NARROW:  # the K >= 64 fp32-MFMA layers too (64 -> 128 of TNet(3) / TNet(64), 64 -> 64, 128 -> C+1)
                self.wide += [self.A[1][0], self.B_tail[0][0], self.B_tail[1][0]]
                # 128 -> C+1 only up to 64 padded columns: as a split-bf16 layer its input is three
                # 128-wide bf16 planes (54 KB in the 64-point build) next to chain D's 256-wide
                # planes (102 KB), which with the biases fills the 160 KB of LDS at N = 64 exactly;
                # a wider last layer reads fp32 rows (34 KB)
                if self.seg and self.D_tail[2][0].shape[1] <= X6_LAST_MAX_N:
                    self.wide.append(self.D_tail[2][0])
            self.frag = {id(w): _frag(w) for w in self.chain_w}
            self.frag6 = {id(w): _frag_x6(w) for w in self.wide}
            # ... and as two fp16 planes with a layer-wide scale, built by ``ensure_f16`` when a forward
            # first takes the fp16 form (``SLICES``; ``_Workspace.uses_f16``): nothing of it exists, and no
            # re-fold pays for it, under NDNET_PN_SLICES=bf16 or where the form never runs
            self.frag16, self.scale16, self.part16 = {}, {}, {}
            self._recipes16 = []  # (w, layer, bn, k0, K) of every split layer (``_fold_jobs``)
            # a layer whose K is a model width (the seg head's global-feature bias, the
            # classification head's conv1: K = F) has it padded to a multiple of 16 with
            # zero rows: the layer then reads g3's padded columns, which chain C leaves at 0
            # (zero weight columns and bias, no ReLU)
            self.fcf = {id(w): _frag(_wT(w.reshape(w.shape[0], -1), _pad(w.shape[1], 16), w.shape[0]))
                        for w in self.fcs}
            # the identity the TNet heads add (ndtnet.py:59), folded into fc3's bias
            self.t1["c3"] = self.t1["c3"] + torch.eye(3, device=dev).reshape(-1)
            self.t2["c3"] = self.t2["c3"] + torch.eye(64, device=dev).reshape(-1)
        self.tensors = _tensors(m)
        # what of the precision settings the fold depends on: which layers have a split-bf16
        # copy.  The mode itself ("x6" / "x3" / "bf16" / "fp32") does not enter: every mode
        # reads these tensors (frag6 or frag), and the argument blocks are kept per mode
        self.prec = (X6_NARROW,)
        self.jobs16 = []  # the fp16 planes' recipes (ndnet_pn_fold16_job), a list of their own beside ``products``
        self.jobs = self._fold_jobs(m)
        self._dev_jobs, self._blocks = None, 0
        self._dev_jobs16, self._units16 = None, 0

    def _fold_seg(self, m, conv) -> None:
        """The segmentation head (chain D and its global-feature bias)."""
        F = self.F
        self.C1 = m.num_classes + 1
        self.s1w, self.s1b = conv(m.conv1, m.bn1)     # [512, 64 + F]
        self.s2w, self.s2b = conv(m.conv2, m.bn2)
        self.s3w, self.s3b = conv(m.conv3, m.bn3)
        self.s4w, self.s4b = m.conv4.weight[:, :, 0].float(), m.conv4.bias.float()
        self.s1a = self.s1w[:, :64].contiguous()      # acts on x_t2
        self.s1bT = self.s1w[:, 64:].t().contiguous()  # [F, 512], acts on g3
        self.s1g = self.s1w[:, 64:].contiguous()       # [512, F] row-major for ndnet_pn_fc_run
        self.D_tail = [(_wT(self.s2w, 512, 256), self.s2b), (_wT(self.s3w, 256, 128), self.s3b),
                       (_wT(self.s4w, 128, _npad(self.C1)), _bpad(self.s4b, _npad(self.C1)))]
        self.s1aT = _wT(self.s1a, 64, 512)                        # seg conv1a W^T [64, 512]
        self.chain_w += [self.s1aT] + [w for w, _ in self.D_tail]
        self.wide += [self.D_tail[0][0], self.D_tail[1][0]]
        self.fcs.append(self.s1g)

    def _fold_cls(self, m) -> None:
        """The classification head (ndtnet.py:188-194: conv1, conv2 with ReLU,
        conv3, softmax; no BatchNorm): conv1 / conv2 as FC layers of
        ndnet_pn_fc_mfma_run, conv3 W^T fragment-major with the classes padded
        to 16 columns for ndnet_pn_cls_head_run, its bias padded with zeros.
        The rows and biases are the parameters themselves ([N, K, 1], as fc3's;
        no view of one is kept: a view made under no_grad breaks a later
        deepcopy of the model once its base has been updated in place)."""
        self.C = m.num_classes
        self.h1w, self.h1b = m.conv1.weight.float(), m.conv1.bias.float()   # [512, F, 1]
        self.h2w, self.h2b = m.conv2.weight.float(), m.conv2.bias.float()   # [256, 512, 1]
        self.h3w = m.conv3.weight.float()                                   # [C, 256, 1]
        self.Cp = _pad(self.C, 16)
        self.h3f = _frag(_wT(self.h3w[:, :, 0], 256, self.Cp))
        self.h3b = _bpad(m.conv3.bias.float(), self.Cp)
        self.fcs += [self.h1w, self.h2w]

    def _fold_jobs(self, m) -> list:
        """The recipe of every tensor above as ndnet_pn_fold_job fields (kind,
        out, layer, BatchNorm, k0, K, Kp, Np, eye): what ``refold`` re-runs in
        place.  Aliases of parameters (fc3 / conv4 weights, conv4 bias) need
        none.  Only for fp32, contiguous parameters (else None: a re-fold
        rebuilds)."""
        if not all(t.dtype == torch.float32 and t.is_contiguous() for t in m.parameters()):
            return None
        fe = m.feature_extractor
        jobs, src = [], {}

        def add(kind, out, layer, bn, k0=0, K=None, Kp=0, Np=0, eye=0):
            ld = layer.weight.shape[1]
            K = ld - k0 if K is None else K
            jobs.append((kind, out, layer, bn, k0, K, Kp, Np, eye))
            src[id(out)] = (layer, bn, k0, K)

        def rows(out, layer, bn, k0=0, K=None):
            add(3, out, layer, bn, k0, K)

        def wt(out, layer, bn, k0=0, K=None):
            add(0, out, layer, bn, k0, K, out.shape[0], out.shape[1])

        def bias(out, layer, bn, eye=0):
            add(5, out, layer, bn, Np=out.shape[0], eye=eye)

        for t, tm, d in ((self.t1, fe.t1, 3), (self.t2, fe.t2, 64)):
            for i in (1, 2, 3):
                conv, bn = getattr(tm, f"conv{i}"), getattr(tm, f"bn{i}")
                rows(t[f"w{i}"], conv, bn)
                bias(t[f"b{i}"], conv, bn)
            rows(t["f1"], tm.fc1, tm.bn4)
            bias(t["c1"], tm.fc1, tm.bn4)
            rows(t["f2"], tm.fc2, tm.bn5)
            bias(t["c2"], tm.fc2, tm.bn5)
            bias(t["c3"], tm.fc3, None, eye=d)
            src[id(t["f3"])] = (tm.fc3, None, 0, tm.fc3.weight.shape[1])  # the parameter itself
        convs = [((self.c1w, self.c1b), fe.conv1, fe.bn1), ((self.c2w, self.c2b), fe.conv2, fe.bn2),
                 ((self.c3w, self.c3b), fe.conv3, fe.bn3)]
        if self.seg:
            convs += [((self.s1w, self.s1b), m.conv1, m.bn1), ((self.s2w, self.s2b), m.conv2, m.bn2),
                      ((self.s3w, self.s3b), m.conv3, m.bn3)]
        for (w, b), conv, bn in convs:
            rows(w, conv, bn)
            bias(b, conv, bn)
        if self.seg:
            rows(self.s1a, m.conv1, m.bn1, 0, 64)
            rows(self.s1g, m.conv1, m.bn1, 64, self.F)
            wt(self.s1bT, m.conv1, m.bn1, 64, self.F)
        for layers, tm in ((self.A, fe.t1), (self.B_tail, fe.t2)):
            for i, (w, _) in enumerate(layers, 1):
                wt(w, getattr(tm, f"conv{i}"), getattr(tm, f"bn{i}"))
        wt(self.C_tail[0], fe.conv3, fe.bn3)
        bias(self.C_tail[1], fe.conv3, fe.bn3)
        if self.seg:
            wt(self.D_tail[0][0], m.conv2, m.bn2)
            wt(self.D_tail[1][0], m.conv3, m.bn3)
            wt(self.D_tail[2][0], m.conv4, None)
            bias(self.D_tail[2][1], m.conv4, None)
        wt(self.c1wT, fe.conv1, fe.bn1)
        wt(self.C_mid[0], fe.conv2, fe.bn2)
        if self.seg:
            wt(self.s1aT, m.conv1, m.bn1, 0, 64)
        else:  # the head's conv1 / conv2 rows are the parameters themselves (no BatchNorm)
            src[id(self.h1w)] = (m.conv1, None, 0, self.F)
            src[id(self.h2w)] = (m.conv2, None, 0, 512)
        if self.baseline:
            wt(self.c1T16, fe.conv1, fe.bn1)
        else:
            add(4, self.t1_basis, fe.conv1, fe.bn1)
        for w in self.chain_w:
            layer, bn, k0, K = src[id(w)]
            add(1, self.frag[id(w)], layer, bn, k0, K, *w.shape)
        for w in self.wide:
            layer, bn, k0, K = src[id(w)]
            add(2, self.frag6[id(w)], layer, bn, k0, K, *w.shape)
            self._recipes16.append((w, layer, bn, k0, K))
        for w in self.fcs:
            layer, bn, k0, K = src[id(w)]
            add(1, self.fcf[id(w)], layer, bn, k0, K, _pad(w.shape[1], 16), w.shape[0])
        if not self.seg:  # conv3 for ndnet_pn_cls_head_run: W^T fragment-major and the bias, classes padded to 16
            add(1, self.h3f, m.conv3, None, 0, 256, 256, self.Cp)
            bias(self.h3b, m.conv3, None)
        return jobs

    def ensure_f16(self) -> bool:
        """The fp16 planes, scales and fold scratch of every split layer, built from the folded weights as
        they are now, with their recipes in ``jobs16`` (a list of their own beside ``products``: every
        later in-place re-fold re-runs them on the device).  Never for the baseline, whose chains stay
        layered.  -> whether the planes exist."""
        if self.frag16 or self.baseline:
            return bool(self.frag16)
        with torch.no_grad():
            for w in self.wide:
                self.frag16[id(w)], self.scale16[id(w)] = _frag_f16(w)
                self.part16[id(w)] = torch.zeros(16, dtype=torch.float32, device=w.device)  # the fold's scratch
        self.jobs16 = [(self.frag16[id(w)], self.part16[id(w)], self.scale16[id(w)], layer, bn, k0, K, *w.shape)
                       for w, layer, bn, k0, K in self._recipes16]
        self._dev_jobs16 = None
        return True

    def can_refold(self, tensors) -> bool:
        """In place: the same parameter / buffer tensors, on a GPU, with the same set of
        split-bf16 layers (any mode: all read the one fold)."""
        return (self.jobs is not None and self.prec == (X6_NARROW,) and self.c1wT.is_cuda
                and len(tensors) == len(self.tensors) and all(a is b for a, b in zip(tensors, self.tensors))
                and all(t.is_contiguous() and t.dtype == torch.float32 for t in tensors if t.is_floating_point()))

    def refold(self) -> None:
        """Every fold above again, from the current weights and running
        statistics, into the same tensors: one ``ndnet_pn_fold_run`` launch on
        the current stream (the workspaces and prebuilt chain argument blocks
        that point at these tensors stay valid)."""
        dev = self.c1wT.device
        if self._dev_jobs is None:
            arr = (_FoldJob * (len(self.jobs) + len(self.products)))()
            for i, (out, a, rhs, bias) in enumerate(self.products, len(self.jobs)):
                J = arr[i]
                assert a.is_contiguous() and rhs.is_contiguous() and rhs.dim() == 2 and out.is_contiguous()
                J.kind, J.out, J.w, J.rhs = 6, out.data_ptr(), a.data_ptr(), rhs.data_ptr()
                J.K, J.ld, J.Np = rhs.shape[0], rhs.shape[0], rhs.shape[1]
                J.N = a.numel() // J.K
                J.bias = bias.data_ptr() if bias is not None else None
                J.out_f64 = 1 if out.dtype == torch.float64 else 0
                assert out.numel() == J.N * J.Np
            for J, (kind, out, layer, bn, k0, K, Kp, Np, eye) in zip(arr, self.jobs):
                J.kind, J.out, J.N, J.K, J.ld, J.k0 = kind, out.data_ptr(), layer.weight.shape[0], K, \
                    layer.weight.shape[1], k0
                J.Kp, J.Np, J.eye = Kp, Np, eye
                if kind == 5:
                    J.bias = layer.bias.data_ptr()
                else:
                    J.w = layer.weight.data_ptr()
                if bn is not None:
                    J.gamma, J.beta = bn.weight.data_ptr(), bn.bias.data_ptr()
                    J.mean, J.var, J.eps = bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.eps
            blocks = ctypes.c_int64()
            _lib.check(_lib.lib().ndnet_pn_fold_prepare(arr, len(arr), ctypes.byref(blocks)), "ndnet_pn_fold_prepare")
            self._dev_jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            self._blocks = blocks.value
        rc = _lib.lib().ndnet_pn_fold_run(self._dev_jobs.data_ptr(), len(self.jobs) + len(self.products),
                                          self._blocks, _lib.stream_ptr(dev))
        _lib.check(rc, "ndnet_pn_fold_run")
        if not self.jobs16:
            return
        # the fp16 planes and their scales from the live weights: two more launches, no host read
        if self._dev_jobs16 is None:
            arr = (_Fold16Job * len(self.jobs16))()
            for J, (out, part, scale, layer, bn, k0, K, Kp, Np) in zip(arr, self.jobs16):
                J.w, J.out, J.partial, J.scale = layer.weight.data_ptr(), out.data_ptr(), part.data_ptr(), scale.data_ptr()
                J.N, J.K, J.ld, J.k0, J.Kp, J.Np = layer.weight.shape[0], K, layer.weight.shape[1], k0, Kp, Np
                if bn is not None:
                    J.gamma, J.var, J.eps = bn.weight.data_ptr(), bn.running_var.data_ptr(), bn.eps
            units = ctypes.c_int64()
            _lib.check(_lib.lib().ndnet_pn_fold16_check(arr, len(arr), ctypes.byref(units)), "ndnet_pn_fold16_check")
            self._dev_jobs16 = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            self._units16 = units.value
        rc = _lib.lib().ndnet_pn_fold16_run(self._dev_jobs16.data_ptr(), len(self.jobs16), self._units16,
                                            _lib.stream_ptr(dev))
        _lib.check(rc, "ndnet_pn_fold16_run")


def _tensors(m) -> list:
    return list(m.parameters()) + list(m.buffers())


def _signature(tensors) -> tuple:
    """Storage and in-place version of every weight: a change re-folds."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def _fc_head(g: torch.Tensor, t: dict, dim: int, h1: torch.Tensor, h2: torch.Tensor, out: torch.Tensor):
    """TNet FC head (ndtnet.py:53-60) into preallocated buffers; the identity is
    folded into t["c3"]."""
    torch.addmm(t["c1"], g, t["f1"].t(), out=h1).relu_()
    torch.addmm(t["c2"], h1, t["f2"].t(), out=h2).relu_()
    torch.addmm(t["c3"], h2, t["f3"].t(), out=out)
    return out.view(-1, dim, dim)


def _build_chain(n: int, in_cols: int, layers, relus, mode: int, gmax=None, out_cols=0, fuse=(),
                 x_ld: int = 12) -> "_Chain":
    """ctypes argument block of one ``ndnet_pn_chain_run`` (x / out set per call).
    ``layers``: (fragment-major weights, per-cloud stride in floats or 0, bias,
    K, N[, prec]) per layer.  Layers in ``fuse`` are produced in 64-column chunks
    straight into the next layer (include/ndnet_pointnet.h)."""
    ch = _Chain()
    ch.x_ld = x_ld
    ch.in_cols = in_cols
    ch.num_points = n
    ch.num_layers = len(layers)
    # LDS regions: layer l reads l & 1, writes (l + 1) & 1; the input tile is
    # zero-filled to the first layer's K; a fused layer's output has no region
    widths = [layers[0][3], 8]
    for i, (w, stride, b, K, N, *prec) in enumerate(layers):
        L = ch.L[i]
        L.prec = prec[0] if prec else 0
        L.w = w.data_ptr()
        L.w_cloud_stride = stride
        L.K, L.N = K, N
        L.bias = b.data_ptr()
        L.bias_cloud_stride = b.stride(0) if b.dim() == 2 else 0
        L.relu = relus[i]
        L.fuse_next = 1 if i in fuse else 0
        if i in fuse:
            continue
        if i + 1 < len(layers) or mode == 1:
            widths[(i + 1) & 1] = max(widths[(i + 1) & 1], N)
    ch.mode = mode
    ch.out_cols = out_cols
    ch.gmax = gmax.data_ptr() if gmax is not None else None
    ch.gmax_ld = gmax.stride(0) if gmax is not None else 0
    ch.max_width, ch.max_width2 = widths
    return ch


# 32-point tiles (ndnet_pn_chain_run_t32) when 64-point tiles would fill at
# most half the CUs (C5's 500-point level: 16 x 8 tiles on 256 CUs); "0" off.
# Always taking them (8-wave workgroups, two per CU, beside other forwards'
# kernels) measured 71-74k against 81k clouds/s (profiles/r03af_t32_ab.txt).
TILE32 = os.environ.get("NDNET_PN_TILE32", "1") == "1"
_cus = {}


def _use_t32(B: int, n: int, device) -> bool:
    if not TILE32:
        return False
    if device not in _cus:
        _cus[device] = torch.cuda.get_device_properties(device).multi_processor_count
    return 2 * B * ((n + 63) // 64) <= _cus[device]


class _Pool12:
    """Argument block of one ``ndnet_pn_pool12_run``: chain C as a per-cloud
    12 -> F layer (include/ndnet_pointnet.h).  It keeps the tensors alive and
    reads their addresses once, as ``_build_chain`` does; the kernel reads
    their contents at every launch, so an in-place re-fold is followed."""

    def __init__(self, ws: "_Workspace", tail: bool = False) -> None:
        W = ws.W
        (w_mid, b_mid), (w_tail, b_tail) = W.C_mid, W.C_tail
        assert w_mid.shape == (64, 128) and w_mid.is_contiguous() and w_tail.shape[0] == 128 and w_tail.is_contiguous()
        self.n, self.F, self.Fp = ws.N, W.F, w_tail.shape[1]
        self.tail = tail  # ``ndnet_pn_pool12_tail_run`` on the fold's W23, b23 (``FOLD_PRODUCTS``)
        head = (ws.w1t2f.data_ptr(), ws.w1t2f.stride(0), ws.b1t2.data_ptr(), ws.b1t2.stride(0))
        if tail:
            assert W.W23.shape == (64, self.Fp) and W.W23.dtype == W.b23.dtype == torch.float64
            self.tensors = (ws.w1t2f, ws.b1t2, W.W23, W.b23, ws.g3)
            self.args = head + (W.W23.data_ptr(), W.b23.data_ptr(), self.Fp, ws.g3.data_ptr(), ws.g3.stride(0))
            return
        self.tensors = (ws.w1t2f, ws.b1t2, w_mid, b_mid, w_tail, b_tail, ws.g3)
        self.args = head + (w_mid.data_ptr(), b_mid.data_ptr(), w_tail.data_ptr(), b_tail.data_ptr(), self.F, self.Fp,
                            ws.g3.data_ptr(), ws.g3.stride(0))


def _run_pool12(blk: "_Pool12", x: torch.Tensor) -> None:
    B, n, _ = x.shape
    assert n == blk.n and x.stride(2) == 1 and x.stride(0) == n * x.stride(1) and x.dtype == torch.float32
    name = "ndnet_pn_pool12_tail_run" if blk.tail else "ndnet_pn_pool12_run"
    rc = getattr(_lib.lib(), name)(x.data_ptr(), x.stride(1), n, *blk.args, B, _lib.stream_ptr(x.device))
    _lib.check(rc, name)


def _run_chain(ch, x: torch.Tensor, out=None) -> None:
    """One per-point launch of the forward: a fused chain (``_Chain``), or
    chain C's 12 -> F form (``_Pool12``)."""
    if isinstance(ch, _Pool12):
        _run_pool12(ch, x)
        return
    assert x.stride(1) == ch.x_ld and x.stride(2) == 1 and x.dtype == torch.float32
    ch.x = x.data_ptr()
    ch.out = out.data_ptr() if out is not None else None
    ext = getattr(ch, "f16", None)  # the fp16 two-slice form (``_Workspace.uses_f16``): the block beside the chain's
    if ext is not None:
        name = "ndnet_pn_chain_f16_run_t32" if _use_t32(x.shape[0], x.shape[1], x.device) else "ndnet_pn_chain_f16_run"
        rc = getattr(_lib.lib(), name)(ctypes.byref(ch), ctypes.byref(ext), x.shape[0], _lib.stream_ptr(x.device))
        _lib.check(rc, name)
        return
    if _use_t32(x.shape[0], x.shape[1], x.device):
        rc = _lib.lib().ndnet_pn_chain_run_t32(ctypes.byref(ch), x.shape[0], _lib.stream_ptr(x.device))
        _lib.check(rc, "ndnet_pn_chain_run_t32")
        return
    rc = _lib.lib().ndnet_pn_chain_run(ctypes.byref(ch), x.shape[0], _lib.stream_ptr(x.device))
    _lib.check(rc, "ndnet_pn_chain_run")


def _chain_torch(x: torch.Tensor, n: int, in_cols: int, layers, relus, mode: int, gmax=None, out=None,
                 out_cols=0, fuse=()) -> None:
    """What one ``ndnet_pn_chain_run`` computes, in torch ops (tests: checks the
    folding algebra on CPU and the kernel against it on the GPU)."""
    h = x[..., :in_cols].float()
    k0 = layers[0][0].shape[-2]
    h = torch.nn.functional.pad(h, (0, k0 - in_cols))
    for i, (w, b) in enumerate(layers):
        h = torch.matmul(h, w[..., : h.shape[-1], :]) + (b[:, None, :] if b.dim() == 2 else b)
        if relus[i]:
            h = torch.relu(h)
    if mode == 0:
        gmax.copy_(torch.maximum(gmax, h.amax(dim=1)))
    else:
        out.copy_(torch.log_softmax(h[..., :out_cols], dim=2))


class _Workspace:
    """Per-(batch, points) intermediates and prebuilt chain argument blocks, so
    an eval forward does no allocation but its output and no struct building.
    The argument blocks are kept per precision mode (``structs[mode]``);
    ``mode`` is the one ``chain`` runs, set by each forward."""

    def __init__(self, W: _Folded, B: int, N: int, dev, mode: str = None) -> None:
        self.W = W
        self.mode = PRECISION if mode is None else mode
        f32 = dict(dtype=torch.float32, device=dev)
        Fp = W.C_tail[0].shape[1]
        # the three max-pooled vectors, -inf before the atomic maxima (ReLU'd maxima are >= 0)
        # -inf before the first forward; the last launch (chain D, or the classification head's
        # ndnet_pn_cls_head_run) re-arms it for the next one
        self.gbuf = torch.full((B, 2048 + Fp), float("-inf"), **f32)
        self.g1, self.g2, self.g3 = self.gbuf[:, :1024], self.gbuf[:, 1024:2048], self.gbuf[:, 2048:]
        self.h1, self.h2 = torch.empty((B, 512), **f32), torch.empty((B, 256), **f32)
        self.t1, self.t2 = torch.empty((B, 9), **f32), torch.empty((B, 4096), **f32)
        self.cvec = torch.empty((B, 512), **f32)        # per-cloud bias of the seg head
        kin = 3 if W.baseline else 12                   # conv1's input columns
        # per-cloud folded weights: plain W^T for the torch emulation ...
        self.w1T = None if W.baseline else torch.empty((B, 12, 64), **f32)  # (W1 M(t1))^T per cloud
        self.w1t2 = torch.empty((B, kin, 64), **f32)    # (W1 M(t1))^T t2: layer 0 of chains C / D
        self.b1t2 = torch.empty((B, 64), **f32)         # b1^T t2
        # ... and fragment-major for the HIP chains (K of conv1 padded 12 -> 16);
        # the HIP chains C / D fold t2 in their prologue (fold_t2)
        self.w1f = None if W.baseline else torch.empty((B, 16 * 64), **f32)
        self.w1t2f = torch.zeros((B, 16 * 64), **f32)   # chain C publishes (W1 M(t1))^T t2 here for chain D
        if W.baseline:
            # the transformed points nan_to_num(t1 p) (ndnet_pn_transform3_run), rows of 4 floats so
            # that chains B-D read them as layer 0's 16-byte row loads; the fourth is never used
            self.xt = torch.zeros((B, N, 4), **f32)
            self.pts = None                             # this forward's points (chain A and the transform read them)
        # chain B collapsed (``collapses_b``), for the torch emulation: (W1 M(t1))^T M per cloud and
        # b1^T M + bM, with (M, bM) TNet(64)'s conv1 (the HIP chain forms both in its prologue)
        self.w1m = None if W.baseline else torch.empty((B, 12, 64), **f32)
        self.b1m = None if W.baseline else torch.empty((64,), **f32)
        first = (W.c1T16, W.c1b) if W.baseline else (self.w1T, W.c1b)
        layered = [  # torch emulation: (in_cols, [(W^T, bias)], relus, mode, kwargs)
            (3, W.A, (1, 1, 1), 0, dict(gmax=self.g1)),
            (kin, [first] + W.B_tail, (0, 1, 1, 1), 0, dict(gmax=self.g2)),
            (kin, [(self.w1t2, self.b1t2), W.C_mid, W.C_tail], (0, 0, 0), 0, dict(gmax=self.g3)),
        ]
        if W.seg:  # the 512-wide seg conv1 output feeds conv2 chunk by chunk (never stored whole)
            layered.append((kin, [(self.w1t2, self.b1t2), (W.s1aT, self.cvec)] + W.D_tail, (0, 1, 1, 1, 0), 1,
                            dict(out_cols=W.C1, fuse=(1,))))
        collapsed = list(layered)  # conv1 and TNet(64)'s conv1 as one layer with its ReLU: three layers
        collapsed[1] = (kin, [(self.w1m, self.b1m)] + W.B_tail[1:], (1, 1, 1), 0, dict(gmax=self.g2))
        self._specs = {(False, False): layered, (True, False): collapsed}
        if W.seg and not W.baseline:
            # chain D collapsed (``collapses_d``): conv1 (t1, t2 folded) and the seg head's conv1[:, :64] as
            # one per-cloud 12 -> 512 layer, wd[b] = w1t2[b] s1aT, with the bias cvec[b] = g3[b] s1g^T + bd[b],
            # bd[b] = b1t2[b] s1aT + s1b (ndnet_pn_fold_seg_run; rows 12..15 of the K = 16 fragment stay zero)
            self.wd = torch.zeros((B, 16 * 512), **f32)
            self.bd = torch.empty((B, 512), **f32)
            self.wdT = torch.empty((B, 12, 512), **f32)  # the same W^T plain, for the torch emulation
            both = list(collapsed)
            both[3] = (kin, [(self.wdT, self.cvec)] + W.D_tail, (1, 1, 1, 0), 1, dict(out_cols=W.C1, fuse=(0,)))
            self._specs[(True, True)] = both
        self.N = N
        self.structs = {}
        self.f16_fallbacks = None  # device counter of the fp16 form's fallback tiles (``take_f16_fallbacks``)
        self.pool12 = None  # chain C's 12 -> F argument block (``uses_pool12``), built at its first launch
        self._pool12 = {}   # ... per form: from the composed tail (``FOLD_PRODUCTS``) or from the layers

    def collapses_b(self, mode: str = None) -> bool:
        """Whether chain B runs conv1 and TNet(64)'s conv1 as one per-cloud 12 -> 64 layer
        (no ReLU separates them, ndtnet.py:149-150 and :47): ``COLLAPSE`` in the "x6" mode,
        whose layers are fp32-accurate, with the 64 -> 64 layer it replaces a split-bf16 one
        (``X6_NARROW``; a non-finite row then leaves both forms as zeros).  Never for the
        baseline, whose transformed points go through a shared conv1."""
        mode = self.mode if mode is None else mode
        return bool(COLLAPSE) and X6_NARROW and not self.W.baseline and mode == "x6"

    def collapses_d(self, mode: str = None) -> bool:
        """Whether chain D opens with conv1 and the seg head's conv1[:, :64] as one per-cloud 12 -> 512
        layer (no ReLU separates them either, ndtnet.py:152-157 and :227-233): where chain B collapses,
        for a segmentation model, with ``ndnet_pn_fold_seg_run`` in ``ndnet_pn_fold_t2_run``'s place (so
        not with NDNET_PN_FOLD_T2=chain, where chain C's prologue publishes chain D's layer 0; its bias
        is ``ndnet_pn_fc_mfma_bias_run``'s, so not with NDNET_PN_FC=gemv).  With one layer fewer in
        front of it, the 512 -> 256 layer's bf16 planes land in the LDS region that also holds the
        logits, which is sized for the wider of the two: past 256 padded classes the 64-point build's
        160 KB no longer hold it (the layered chain keeps the planes beside the logits and takes up to
        ``MAX_LAST_N``), so such a model keeps chain D layered."""
        return (self.collapses_b(mode) and self.W.seg and FOLD_T2_KERNEL and FC_MFMA
                and _npad(self.W.C1) <= COLLAPSE_D_MAX_LAST_N)

    @property
    def specs(self) -> list:
        """The chains of the current mode for the torch emulation."""
        return self._specs[(self.collapses_b(), self.collapses_d())]

    def uses_pool12(self) -> bool:
        """Whether chain C runs as one ``ndnet_pn_pool12_run`` in the current mode.
        Only where the layers are fp32-accurate ("x6", "fp32": the reduced modes
        are defined layer by layer and keep the chain), conv1 has per-cloud
        weights that ``ndnet_pn_fold_t2_run`` has already folded t2 into (not the
        baseline; not NDNET_PN_FOLD_T2=chain, where chain C's prologue is what
        publishes them for chain D), and NDNET_PN_BACKBONE is not "chain"."""
        return BACKBONE == "pool12" and FOLD_T2_KERNEL and not self.W.baseline and self.mode in ("x6", "fp32")

    def uses_tail(self) -> bool:
        """Whether that launch starts from the fold's composed tail (``ndnet_pn_pool12_tail_run`` on
        ``W.W23``, ``W.b23``): ``FOLD_PRODUCTS``, wherever ``uses_pool12`` holds.  Not with
        NDNET_PN_COLLAPSE=0, which keeps the forward as it was before either change, launch for launch
        and bit for bit."""
        return bool(FOLD_PRODUCTS) and bool(COLLAPSE) and self.uses_pool12()

    def uses_f16(self) -> bool:
        """Whether the chains' split layers run in the fp16 two-slice form (``SLICES``): only in the "x6"
        mode's default forward -- the composed tail, chain B collapsed and, for a segmentation model,
        chain D collapsed.  With any of NDNET_PN_COLLAPSE=0, NDNET_PN_FOLD_PRODUCTS=0,
        NDNET_PN_BACKBONE=chain, NDNET_PN_FOLD_T2=chain, a many-classes model, the baseline or a reduced
        mode, the forward is the bf16 three-slice one, launch for launch and bit for bit."""
        return (SLICES == "f16" and self.mode == "x6" and self.uses_tail() and self.collapses_b()
                and (not self.W.seg or self.collapses_d()) and self.W.ensure_f16())

    def take_f16_fallbacks(self) -> int:
        """Tiles that left fp16's window and ran the bf16 form since the last call (it waits for the
        current stream; 0 when no forward of this workspace ran the fp16 form)."""
        if self.f16_fallbacks is None:
            return 0
        rc = _lib.lib().ndnet_pn_take_f16_fallbacks(self.f16_fallbacks.data_ptr(),
                                                    _lib.stream_ptr(self.f16_fallbacks.device))
        if rc < 0:
            _lib.check(rc, "ndnet_pn_take_f16_fallbacks")
        return rc

    def hip_layers(self, mode: str) -> list:
        """The chains' layers (A-D; A-C for a classification model) for ``_build_chain`` in one precision mode:
        every layer with a split-bf16 copy takes the mode's prec (all modes
        read the same ``frag6``); "fp32" and the other layers read ``frag``."""
        W = self.W

        def shared(wb):
            w, b = wb
            if mode != "fp32" and id(w) in W.frag6:
                return (W.frag6[id(w)], 0, b, w.shape[0], w.shape[1], MODES[mode], w)  # w: the layer, for ``uses_f16``
            return (W.frag[id(w)], 0, b, w.shape[0], w.shape[1])

        # conv1: per cloud with t1 folded in; the baseline's is the shared layer (t1 went into the points)
        L1 = shared((W.c1T16, W.c1b)) if W.baseline else (self.w1f, self.w1f.stride(0), W.c1b, 16, 64)
        # chain C's layer 0: conv1 with t1 and t2 folded (ndnet_pn_fold_t2_run), or
        # with t1 only and t2 folded in its prologue (NDNET_PN_FOLD_T2=chain; always for the
        # baseline, whose conv1 has no per-cloud copy for ndnet_pn_fold_t2_run to read)
        LC = (self.w1t2f, self.w1t2f.stride(0), self.b1t2, 16, 64) if FOLD_T2_KERNEL and not W.baseline else L1
        # chain B collapsed: layer 0 is conv1 (its prologue folds TNet(64)'s conv1 in, ``chain``)
        layers = [
            [shared(x) for x in W.A],
            [L1] + [shared(x) for x in W.B_tail[1 if self.collapses_b(mode) else 0:]],
            [LC, shared(W.C_mid), shared(W.C_tail)],
        ]
        if W.seg and self.collapses_d(mode):  # 12 -> 512 per cloud on the fp32 MFMA, fused into 512 -> 256
            layers.append([(self.wd, self.wd.stride(0), self.cvec, 16, 512)] + [shared(x) for x in W.D_tail])
        elif W.seg:
            layers.append([(self.w1t2f, self.w1t2f.stride(0), self.b1t2, 16, 64), shared((W.s1aT, self.cvec))] +
                          [shared(x) for x in W.D_tail])
        return layers

    def chain(self, i: int, x: torch.Tensor, chain_fn=None, out=None) -> None:
        in_cols, layers, relus, mode, kw = self.specs[i]
        if chain_fn is not None:
            kw = dict(kw)
            if out is not None:
                kw["out"] = out
            chain_fn(x, self.N, in_cols, layers, relus, mode, **kw)
            return
        W = self.W
        collapse_b, collapse_d = self.collapses_b(), self.collapses_d()
        # argument blocks per mode and form
        f16 = self.uses_f16()
        skey = self.mode if not collapse_b else (self.mode, "collapse B+D" if collapse_d else "collapse B")
        if f16:
            skey = skey + ("f16",)
        structs = self.structs.get(skey)
        if structs is None:
            # input rows: [B,N,12] blocks; the baseline's chain A reads the points themselves, B-D ws.xt
            x_lds = (3, 4, 4, 4) if W.baseline else (12, 12, 12, 12)
            hls = self.hip_layers(self.mode)
            structs = self.structs[skey] = [_build_chain(self.N, s[0], hl, s[2], s[3], x_ld=xl, **s[4])
                                            for s, hl, xl in zip(self.specs, hls, x_lds)]
            if f16:
                # every chain with split layers (chain C is the 12 -> F launch here) takes the fp16 block
                # beside its own: the planes and scale of each split layer, and this workspace's counter
                if self.f16_fallbacks is None:
                    self.f16_fallbacks = torch.zeros(1, dtype=torch.int32, device=self.gbuf.device)
                for blk, hl in zip(structs, hls):
                    if not any(len(t) == 7 for t in hl):
                        continue
                    ext = _F16()
                    for l, t in enumerate(hl):
                        if len(t) == 7:
                            ext.w16[l] = W.frag16[id(t[6])].data_ptr()
                            ext.scale[l] = W.scale16[id(t[6])].data_ptr()
                    ext.fallbacks = self.f16_fallbacks.data_ptr()
                    blk.f16 = ext
            if W.seg:  # the last chain re-arms the max-pool buffer (-inf) for the next forward
                structs[3].clear = self.gbuf.data_ptr()
                structs[3].clear_count = self.gbuf.numel()
            if HEAD3_IN_CHAIN and not W.baseline:  # chain B computes t1 and its conv1 weights itself
                cb = structs[1]
                cb.head_h2, cb.head_ld, cb.head_K = self.h2.data_ptr(), self.h2.stride(0), self.h2.shape[1]
                cb.head_w3, cb.head_b3 = W.t1["f3"].data_ptr(), W.t1["c3"].data_ptr()
                cb.head_basis, cb.head_kin, cb.head_nout = W.t1_basis.data_ptr(), 12, 64
                cb.head_t1 = self.t1.data_ptr()
            if collapse_b:
                # chain B: TNet(64)'s conv1 (M, bM: shared, hot) folded through conv1 in the prologue,
                # after the head prologue -- layer 0 = relu(x (W1f[b] M) + (b1 M + bM)).  Formed from
                # the live folded tensors at every launch: an in-place re-fold is followed
                cb = structs[1]
                m_w, m_b = W.B_tail[0]
                assert m_w.shape == (64, 64) and m_w.is_contiguous() and m_b.shape == (64,)
                cb.fold_t2, cb.fold_ld, cb.fold_bias = m_w.data_ptr(), 0, m_b.data_ptr()
                cb.x_nonfinite_nan = 1  # a NaN / inf row leaves the first ReLU as zeros, as the layered pair's
            if collapse_d:
                structs[3].x_nonfinite_nan = 1
            if not FOLD_T2_KERNEL or W.baseline:  # chain C: t2 through layer 0 (prologue fold), published for chain D
                cc = structs[2]
                cc.fold_t2, cc.fold_ld = self.t2.data_ptr(), self.t2.stride(0)
                cc.fold_out_w, cc.fold_out_b = self.w1t2f.data_ptr(), self.b1t2.data_ptr()
        blk = structs[i]
        if i == 2 and self.uses_pool12():  # chain C collapsed to its 12 -> F layer: one launch in the chain's place
            tail = self.uses_tail()
            if tail not in self._pool12:
                self._pool12[tail] = _Pool12(self, tail)
            blk = self.pool12 = self._pool12[tail]
        if chain_timing is not None:  # torch events on the launch stream (bench.py)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _run_chain(blk, x, out)
            e1.record()
            chain_timing.append((i, e0, e1))
        else:
            _run_chain(blk, x, out)


def _folded(model):
    """The model's folded weights, re-folded when any weight changed."""
    cache = model._hip
    if cache is None:
        tensors = _tensors(model)
        cache = model._hip = {"tensors": tensors, "sig": None, "stale": False}
    sig = _signature(cache["tensors"])
    cur = _tensors(model)  # a parameter or buffer replaced by another tensor is a change too
    replaced = len(cur) != len(cache["tensors"]) or any(a is not b for a, b in zip(cur, cache["tensors"]))
    if replaced or cache["sig"] != sig or cache["stale"]:
        # stale: the model was in train mode since the last fold, where a
        # replayed training graph updates the weights without bumping their
        # versions (ndnet.training.GraphedTrainStep)
        W = cache.get("W")
        if W is not None and W.can_refold(_tensors(model)):
            W.refold()  # one launch, in place: workspaces and argument blocks stay valid
        else:
            cache.update(tensors=_tensors(model), W=_Folded(model), ws={})
            sig = _signature(cache["tensors"])
        cache.update(sig=sig, stale=False)
    return cache


# TNet(64)'s transform through conv1 (layer 0 of chains C and D): "kernel"
# (default, round 5) once per cloud by ndnet_pn_fold_t2_run after fc3; "chain"
# in chain C's prologue, every workgroup (fold_t2), published for chain D
FOLD_T2_KERNEL = os.environ.get("NDNET_PN_FOLD_T2", "kernel") == "kernel"
# Chain C (conv1 with t1 and t2 folded, conv2, conv3, max: no ReLU anywhere):
# "pool12" (default) runs it as one per-cloud 12 -> F layer, ndnet_pn_pool12_run
# (9,216 fp32 multiply-adds per point at F = 768 where the layered chain does
# 106,496 split-bf16 ones), wherever ``_Workspace.uses_pool12`` allows; "chain"
# keeps the layered k_pn_chain launch everywhere (A/B runs)
BACKBONE = os.environ.get("NDNET_PN_BACKBONE", "pool12")
if BACKBONE not in ("pool12", "chain"):
    raise ValueError(f"NDNET_PN_BACKBONE must be 'pool12' or 'chain', not {BACKBONE!r}")
# Chain B's first two layers, conv1 (t1 folded) and TNet(64)'s conv1, have no ReLU between them
# (ndtnet.py:149-150, :47): "1" (default) runs them as one per-cloud 12 -> 64 VALU layer whose
# weights chain B's prologue composes (ndnet_pn_chain.fold_t2 with a shared matrix and fold_bias),
# wherever ``_Workspace.collapses_b`` allows; and chain D's conv1 (t1, t2 folded) and the seg head's
# conv1[:, :64] as one per-cloud 12 -> 512 layer on the fp32 MFMA (``_Workspace.collapses_d``).
# "0" keeps the layered launches, bit for bit.  A module attribute read when a forward picks its
# argument blocks, like BACKBONE.
COLLAPSE = os.environ.get("NDNET_PN_COLLAPSE", "1") == "1"
# Weight-only products formed by the fold (NDNET_FOLD_PROD jobs, re-run by every in-place re-fold) where
# the forward formed them at every launch: "1" (default) runs chain C's 12 -> F launch from the composed
# tail W23 = W2'^T W3'^T, b23 (ndnet_pn_pool12_tail_run) wherever ``_Workspace.uses_tail`` allows; "0"
# keeps ndnet_pn_pool12_run, bit for bit.  A module attribute read when a forward picks its argument
# blocks, like BACKBONE.
FOLD_PRODUCTS = os.environ.get("NDNET_PN_FOLD_PRODUCTS", "1") == "1"
# The slices of the x6 mode's split layers: "f16" (default) runs them as two fp16 slices and three products
# per operand pair (ndnet_pn_chain_f16_run: half of x6's matrix instructions in the same accuracy class),
# each tile falling back to the bf16 three-slice code when its activations leave fp16's window, wherever
# ``_Workspace.uses_f16`` allows; "bf16" keeps ndnet_pn_chain_run everywhere, bit for bit.  A module
# attribute read when a forward picks its argument blocks, like BACKBONE.
def _slices(value: str) -> str:
    if value not in ("f16", "bf16"):
        raise ValueError(f"NDNET_PN_SLICES must be 'f16' or 'bf16', not {value!r}")
    return value


SLICES = _slices(os.environ.get("NDNET_PN_SLICES", "f16"))
# TNet(3)'s tail (fc3 + the t1 fold of conv1): "chain" (default) computes it in
# chain B's prologue, per workgroup (ndnet_pn_chain.head_*: one launch and one
# boundary fewer); "kernel" runs ndnet_pn_head3_run before chain B
HEAD3_IN_CHAIN = os.environ.get("NDNET_PN_HEAD3", "chain") == "chain"

# TNet / seg-bias FC layers: "mfma" (default: ndnet_pn_fc_mfma_run, 16-row
# fp32-MFMA GEMM over fragment-major weights) or "gemv" (ndnet_pn_fc_run,
# VALU dot products over row-major weights).  Round 3 also tried a TNet head's
# 2-3 layers in ONE launch handing off through an in-memory counter (stage
# workgroups polling, sc1 stores / loads): the forward's non-chain time rose
# from 46 to 63 us (profiles/r03z_fc_ab.txt), so every layer stays a launch.
FC_MFMA = os.environ.get("NDNET_PN_FC", "mfma") == "mfma"


def _fc(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, relu: bool, wf=None) -> None:
    """out = act(x @ w^T + b) on a HIP kernel (chunks of 16 clouds); wf: W^T
    fragment-major (the MFMA kernel; its K is w's padded to a multiple of 16
    with zero rows, and x's row must be readable -- and finite -- that far),
    else the GEMV kernel on w."""
    B = x.shape[0]
    st = _lib.stream_ptr(x.device)
    for c0 in range(0, B, 16):
        n = min(16, B - c0)
        if FC_MFMA and wf is not None:
            rc = _lib.lib().ndnet_pn_fc_mfma_run(x[c0].data_ptr(), x.stride(0), wf.data_ptr(), b.data_ptr(),
                                                 out[c0].data_ptr(), out.stride(0), n, _pad(w.shape[1], 16),
                                                 w.shape[0], 1 if relu else 0, st)
            _lib.check(rc, "ndnet_pn_fc_mfma_run")
        else:
            rc = _lib.lib().ndnet_pn_fc_run(x[c0].data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(),
                                            out[c0].data_ptr(), out.stride(0), n, w.shape[1], w.shape[0],
                                            1 if relu else 0, st)
            _lib.check(rc, "ndnet_pn_fc_run")


def _glue_hip(W, ws, B: int):
    """The per-cloud steps as HIP kernels: TNet heads (fc1, fc2, fc3 + I) and the
    weight folds (t1 into conv1, t2 into conv2 / seg conv1)."""
    st = lambda: _lib.stream_ptr(ws.gbuf.device)  # noqa: E731

    def fc(x, w, b, out, relu):  # with the layer's fragment-major weights (the MFMA kernel)
        _fc(x, w, b, out, relu, W.fcf.get(id(w)))

    def head_a():
        t = W.t1
        fc(ws.g1, t["f1"], t["c1"], ws.h1, True)
        fc(ws.h1, t["f2"], t["c2"], ws.h2, True)
        if HEAD3_IN_CHAIN:  # fc3 and the t1 fold run in chain B's prologue
            return
        for c0 in range(0, B, 16):
            n = min(16, B - c0)
            rc = _lib.lib().ndnet_pn_head3_run(ws.h2[c0].data_ptr(), ws.h2.stride(0), t["f3"].data_ptr(),
                                               t["c3"].data_ptr(), W.t1_basis.data_ptr(), ws.t1[c0].data_ptr(),
                                               ws.w1f[c0].data_ptr(), n, 256, 12, 64, st())
            _lib.check(rc, "ndnet_pn_head3_run")

    def head_a_points():
        # the baseline: t1 itself (fc3 on the GEMV kernel: 9 outputs, row-major weights), then
        # nan_to_num(t1 p) for every point -- not linear, so a launch of its own (no fold into conv1)
        t = W.t1
        fc(ws.g1, t["f1"], t["c1"], ws.h1, True)
        fc(ws.h1, t["f2"], t["c2"], ws.h2, True)
        _fc(ws.h2, t["f3"], t["c3"], ws.t1, False, None)
        rc = _lib.lib().ndnet_pn_transform3_run(ws.pts.data_ptr(), ws.pts.stride(1), ws.t1.data_ptr(),
                                                ws.xt.data_ptr(), ws.xt.stride(1), B, ws.pts.shape[1], st())
        _lib.check(rc, "ndnet_pn_transform3_run")

    def head_b():
        t = W.t2
        fc(ws.g2, t["f1"], t["c1"], ws.h1, True)
        fc(ws.h1, t["f2"], t["c2"], ws.h2, True)
        fc(ws.h2, t["f3"], t["c3"], ws.t2, False)  # t2
        if ws.collapses_d():  # the same, and the seg head's conv1 through it: chain D's first layer (wd, bd)
            assert W.s1aT.shape == (64, 512) and W.s1aT.is_contiguous()
            rc = _lib.lib().ndnet_pn_fold_seg_run(ws.w1f.data_ptr(), ws.w1f.stride(0), W.c1b.data_ptr(),
                                                  ws.t2.data_ptr(), ws.t2.stride(0), ws.w1t2f.data_ptr(),
                                                  ws.b1t2.data_ptr(), W.s1aT.data_ptr(), W.s1b.data_ptr(), 512,
                                                  ws.wd.data_ptr(), ws.wd.stride(0), ws.bd.data_ptr(),
                                                  ws.bd.stride(0), B, st())
            _lib.check(rc, "ndnet_pn_fold_seg_run")
        elif FOLD_T2_KERNEL and not W.baseline:  # t2 through conv1: chains C / D's layer 0, once per cloud
            rc = _lib.lib().ndnet_pn_fold_t2_run(ws.w1f.data_ptr(), ws.w1f.stride(0), W.c1b.data_ptr(),
                                                 ws.t2.data_ptr(), ws.t2.stride(0), ws.w1t2f.data_ptr(),
                                                 ws.b1t2.data_ptr(), B, st())
            _lib.check(rc, "ndnet_pn_fold_t2_run")

    def seg_bias():
        if not ws.collapses_d():
            fc(ws.g3[:, : W.F], W.s1g, W.s1b, ws.cvec, False)
            return
        # chain D collapsed: the bias row of each cloud is bd[b] (which holds s1b), ndnet_pn_fold_seg_run's
        wf = W.fcf[id(W.s1g)]
        for c0 in range(0, B, 16):
            rc = _lib.lib().ndnet_pn_fc_mfma_bias_run(ws.g3[c0].data_ptr(), ws.g3.stride(0), wf.data_ptr(),
                                                      ws.bd[c0].data_ptr(), ws.bd.stride(0), ws.cvec[c0].data_ptr(),
                                                      ws.cvec.stride(0), min(16, B - c0), _pad(W.F, 16), 512, 0, st())
            _lib.check(rc, "ndnet_pn_fc_mfma_bias_run")

    def cls_head(out):
        # g3's columns past F are chain C's zero padding, matched by zero weight rows
        fc(ws.g3[:, : W.F], W.h1w, W.h1b, ws.h1, True)
        fc(ws.h1, W.h2w, W.h2b, ws.h2, True)
        rc = _lib.lib().ndnet_pn_cls_head_run(ws.h2.data_ptr(), ws.h2.stride(0), W.h3f.data_ptr(), W.h3b.data_ptr(),
                                              out.data_ptr(), out.stride(0), None, 0, B, ws.h2.shape[1], W.Cp, W.C,
                                              ws.gbuf.data_ptr(), ws.gbuf.numel(), st())
        _lib.check(rc, "ndnet_pn_cls_head_run")

    return (head_a_points if W.baseline else head_a), head_b, (seg_bias if W.seg else cls_head)


def _glue_torch(W, ws, B: int):
    """The same steps as torch ops (the emulation path of the tests)."""
    def head_a():
        t1 = _fc_head(ws.g1, W.t1, 3, ws.h1, ws.h2, ws.t1)
        torch.matmul(t1.reshape(B, 9), W.t1_basis, out=ws.w1T.view(B, 12 * 64))
        if ws.collapses_b():  # chain B's composed layer 0 (the HIP chain's prologue)
            m_w, m_b = W.B_tail[0]
            torch.matmul(ws.w1T, m_w, out=ws.w1m)
            torch.addmv(m_b, m_w.t(), W.c1b, out=ws.b1m)

    def head_a_points():
        t1 = _fc_head(ws.g1, W.t1, 3, ws.h1, ws.h2, ws.t1)
        ws.xt[..., :3] = torch.nan_to_num(torch.bmm(ws.pts, t1.transpose(1, 2)), nan=0.0)

    def head_b():
        t2 = _fc_head(ws.g2, W.t2, 64, ws.h1, ws.h2, ws.t2)
        torch.matmul(W.c1wT if W.baseline else ws.w1T, t2, out=ws.w1t2)
        torch.matmul(W.c1b[None, None, :], t2, out=ws.b1t2.view(B, 1, 64))
        if ws.collapses_d():  # chain D's composed first layer (ndnet_pn_fold_seg_run)
            torch.matmul(ws.w1t2, W.s1aT, out=ws.wdT)
            torch.addmm(W.s1b, ws.b1t2, W.s1aT, out=ws.bd)

    def seg_bias():
        torch.addmm(ws.bd if ws.collapses_d() else W.s1b, ws.g3[:, : W.F], W.s1bT, out=ws.cvec)

    def cls_head(out):
        torch.addmm(W.h1b, ws.g3[:, : W.F], W.h1w[:, :, 0].t(), out=ws.h1).relu_()
        torch.addmm(W.h2b, ws.h1, W.h2w[:, :, 0].t(), out=ws.h2).relu_()
        out.copy_(torch.softmax(torch.addmm(W.h3b[: W.C], ws.h2, W.h3w[:, :, 0].t()), dim=1))

    return (head_a_points if W.baseline else head_a), head_b, (seg_bias if W.seg else cls_head)


# Workspace slot of the forwards launched from now on (``workspace_slot``).
_slot = 0


class workspace_slot:
    """``with workspace_slot(i):`` -- forwards launched inside use workspace
    slot ``i`` of their shape.  A forward's workspace (the max-pool buffer
    that chain D re-arms, the FC-head intermediates, the per-cloud folded
    weights and the prebuilt argument blocks) is cached per (batch, points,
    device, slot) and is written by every forward of that key, so forwards
    that may run CONCURRENTLY -- launched on different streams with no order
    between them, e.g. two halves of a batch captured on two streams of one
    graph -- must use different slots; forwards in stream order may share one
    (the default slot 0).  This was the hazard behind round 2's crashed
    two-stream capture: both halves shared one slot, so one half's chain D
    re-armed the max-pool buffer the other half was still reducing into."""

    def __init__(self, slot: int) -> None:
        self.slot, self.prev = int(slot), None

    def __enter__(self):
        global _slot
        self.prev, _slot = _slot, self.slot
        return self

    def __exit__(self, *exc):
        global _slot
        _slot = self.prev
        return False


def _features(model, points: torch.Tensor, covariances: torch.Tensor, chain):
    """What both forwards share: the fold, the workspace of this shape and
    slot, the [B,N,12] input block, and chains A, B and C with the per-cloud
    steps between them.  Leaves the pooled global feature in ``ws.g3`` and
    returns (W, ws, x, the glue's last step)."""
    mode = model_precision(model)
    cache = _folded(model)
    W = cache["W"]
    B, N, _ = points.shape
    dev = points.device
    key = (B, N, dev, _slot)
    ws = cache["ws"].get(key)
    if ws is None:
        ws = cache["ws"][key] = _Workspace(W, B, N, dev, mode)
    ws.mode = mode  # the model's mode as of this forward: its argument blocks are kept per mode
    if W.baseline:
        # chain A and the transform read the points ([B,N,3] rows of 3), chains B-D the transformed ones
        xa = ws.pts = points.float().contiguous()
        x = ws.xt
    # one [B,N,12] block; ndt_preprocessing already returns views of one
    elif (points.stride() == (N * 12, 12, 1) and covariances.stride() == (N * 12, 12, 1)
            and covariances.data_ptr() == points.data_ptr() + 12 and points.dtype == torch.float32):
        xa = x = points.as_strided((B, N, 12), (N * 12, 12, 1))
    else:
        xa = x = torch.cat((points, covariances), dim=2).float().contiguous()
    head_a, head_b, last = (_glue_hip if chain is None else _glue_torch)(W, ws, B)
    if chain is not None:
        ws.gbuf.fill_(float("-inf"))
    ws.chain(0, xa, chain)  # A: TNet(3) -> g1
    head_a()                # t1, (W1 M(t1))^T
    ws.chain(1, x, chain)   # B: conv1 (+t1) then TNet(64) -> g2
    head_b()                # t2, t2 @ [W2^T | Ws1a^T]
    ws.chain(2, x, chain)   # C: conv2, conv3, max over points -> g3
    return W, ws, x, last


def segmentation_forward(model, points: torch.Tensor, covariances: torch.Tensor, chain=None) -> torch.Tensor:
    """model(points [B,N,3], covariances [B,N,9]) -> log-probs [B,N,C+1], eval mode.

    The split-bf16 layers run in the model's precision mode as of this call
    (``model_precision``).  ``chain``: None runs every step on the HIP kernels; a chain emulator
    (``_chain_torch``) runs the chains and the per-cloud steps as torch ops.
    Concurrent forwards (different streams, no order) need different
    ``workspace_slot``s."""
    W, ws, x, seg_bias = _features(model, points, covariances, chain)
    B, N, _ = points.shape
    seg_bias()              # the broadcast global feature as a per-cloud bias of the seg head
    out = torch.empty((B, N, W.C1), dtype=torch.float32, device=points.device)
    ws.chain(3, x, chain, out=out)
    if chain is not None:
        ws.gbuf.fill_(float("-inf"))  # the HIP path expects it armed (chain D re-arms it there)
    return out


def classification_forward(model, points: torch.Tensor, covariances: torch.Tensor, chain=None) -> torch.Tensor:
    """model(points [B,N,3], covariances [B,N,9]) -> class probabilities
    [B, num_classes, 1] (the reference's shape, ndtnet.py:188-196), eval mode.

    Chains A-C, the per-cloud steps, the workspace (same cache key and
    ``workspace_slot``) and the precision modes are ``segmentation_forward``'s;
    the head -- relu(conv1), relu(conv2) on ``ndnet_pn_fc_mfma_run``, then conv3
    and the softmax in one ``ndnet_pn_cls_head_run``, which also re-arms the
    max-pool buffer -- stays on the fp32 MFMA in every mode.  ``chain``: as for
    ``segmentation_forward`` (the head then runs as torch ops too)."""
    W, ws, x, cls_head = _features(model, points, covariances, chain)
    out = torch.empty((points.shape[0], W.C), dtype=torch.float32, device=points.device)
    cls_head(out)
    if chain is not None:
        ws.gbuf.fill_(float("-inf"))  # the HIP path expects it armed (the head kernel re-arms it there)
    return out.unsqueeze(2)
