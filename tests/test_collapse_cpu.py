"""Chain B with TNet(64)'s first layer collapsed into conv1, and chain D with
the seg head's conv1 collapsed into its first layer (NDNET_PN_COLLAPSE,
``pointnet_hip.COLLAPSE``): the collapsed ``specs`` of both chains against the
layered ones through ``pointnet_hip._chain_torch`` in float64, the emulated
forwards against each other, the argument rules of the new ``ndnet_pn_chain``
fields on host memory (a rejected block is never launched), and the ctypes
mirror of the struct against include/ndnet_pointnet.h.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from model_init import deterministic_state

B, N, F = 3, 77, 64


class _F64(torch.Tensor):
    """``_chain_torch`` takes its input with ``.float()``; this input stays float64."""

    def float(self):
        return self.as_subclass(torch.Tensor).double()


def _model(kind):
    from ndnet.models.ndtnet import NDTNetClassification, NDTNetSegmentation
    m = NDTNetSegmentation(3, 5, F) if kind == "seg" else NDTNetClassification(3, 7, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.eval()


def _inputs():
    g = torch.Generator().manual_seed(F + N)
    return torch.rand((B, N, 3), generator=g) * 20 - 10, torch.randn((B, N, 9), generator=g)


def _forward(ph, kind, m, p, c, chain=None):
    fwd = ph.segmentation_forward if kind == "seg" else ph.classification_forward
    with torch.no_grad():
        return fwd(m, p, c, chain=chain or ph._chain_torch)


@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_collapsed_specs_equal_the_layered_ones_in_float64(monkeypatch, kind):
    from ndnet.models import pointnet_hip as ph
    monkeypatch.setattr(ph, "COLLAPSE", True)
    monkeypatch.setattr(ph, "PRECISION", "x6")
    m = _model(kind)
    p, c = _inputs()
    _forward(ph, kind, m, p, c)  # fills the per-cloud conv1 (w1T) and its composition (w1m, b1m)
    (ws,) = m._hip["ws"].values()
    assert ws.collapses_b() and ws.collapses_d() == (kind == "seg")
    lay, col = ws._specs[(False, False)], ws.specs
    assert all((a is b) == (i not in (1, 3)) for i, (a, b) in enumerate(zip(lay, col))), "chains B and D change"
    (_, l_layers, l_relus, l_mode, _), (_, c_layers, c_relus, c_mode, _) = lay[1], col[1]
    assert l_relus == (0, 1, 1, 1) and c_relus == (1, 1, 1) and l_mode == c_mode == 0
    assert len(c_layers) == 3 and all(a[0] is b[0] and a[1] is b[1] for a, b in zip(l_layers[2:], c_layers[1:]))
    # the composition in float64 from the layered chain's own first two layers
    (w1, b1), (mw, mb) = l_layers[0], l_layers[1]
    w64 = w1.double() @ mw.double()
    b64 = b1.double() @ mw.double() + mb.double()
    x = torch.cat((p, c), dim=2).double().as_subclass(_F64)
    out = {}
    for name, layers, relus in (("layered", [(w.double(), b.double()) for w, b in l_layers], l_relus),
                                ("collapsed", [(w64, b64)] + [(w.double(), b.double()) for w, b in c_layers[1:]], c_relus)):
        g = torch.full((B, 1024), float("-inf"), dtype=torch.float64)
        ph._chain_torch(x, N, 12, layers, relus, 0, gmax=g)
        assert g.dtype == torch.float64
        out[name] = g
    err = (out["layered"] - out["collapsed"]).abs().max().item()
    scale = out["layered"].abs().max().item()
    print(f"{kind}: collapsed vs layered chain B in float64 {err:.3e} (|g2| <= {scale:.3g})")
    assert err <= 1e-12 * max(scale, 1.0)
    # what the emulation's glue composed in fp32: 64 products per element, each factor rounded once
    e_w = (ws.w1m.double() - w64).abs().max().item()
    e_b = (ws.b1m.double() - b64).abs().max().item()
    lim_w = 66 * 2.0 ** -24 * (w1.double().abs() @ mw.double().abs()).max().item()
    lim_b = 67 * 2.0 ** -24 * ((b1.double().abs() @ mw.double().abs()) + mb.double().abs()).max().item()
    print(f"{kind}: fp32 composition off by {e_w:.3e} (<= {lim_w:.3e}), bias {e_b:.3e} (<= {lim_b:.3e})")
    assert e_w <= lim_w and e_b <= lim_b


def test_collapsed_chain_d_equals_the_layered_one_in_float64(monkeypatch):
    """Chain D of the seg model (mode 1, log-probs): layered (w1t2, b1t2), (s1aT, g3 s1g^T + s1b), ... with
    relus (0, 1, 1, 1, 0) against the collapsed wd = w1t2 s1aT with the bias row g3 s1g^T + bd, bd = b1t2 s1aT
    + s1b, relus (1, 1, 1, 0), both through ``_chain_torch`` in float64 from the fp32 values of one forward."""
    from ndnet.models import pointnet_hip as ph
    monkeypatch.setattr(ph, "COLLAPSE", True)
    monkeypatch.setattr(ph, "PRECISION", "x6")
    m = _model("seg")
    p, c = _inputs()
    seen = {}

    def chain(x, n, in_cols, layers, relus, mode, **kw):
        if mode == 1:  # chain D: the pooled backbone feature before the forward re-arms its buffer
            (ws,) = m._hip["ws"].values()
            seen["g3"] = ws.g3.clone()
        return ph._chain_torch(x, n, in_cols, layers, relus, mode, **kw)

    _forward(ph, "seg", m, p, c, chain=chain)
    (ws,) = m._hip["ws"].values()
    W = ws.W
    assert ws.collapses_d()
    (_, l_layers, l_relus, l_mode, l_kw), (_, c_layers, c_relus, c_mode, c_kw) = ws._specs[(False, False)][3], ws.specs[3]
    assert l_relus == (0, 1, 1, 1, 0) and c_relus == (1, 1, 1, 0) and l_mode == c_mode == 1
    assert l_kw == dict(out_cols=W.C1, fuse=(1,)) and c_kw == dict(out_cols=W.C1, fuse=(0,))
    assert len(c_layers) == 4 and all(a[0] is b[0] and a[1] is b[1] for a, b in zip(l_layers[2:], c_layers[1:]))
    assert c_layers[0][0] is ws.wdT and c_layers[0][1] is ws.cvec and l_layers[1][1] is ws.cvec
    (w1t2, b1t2), s1aT = l_layers[0], l_layers[1][0]
    assert w1t2 is ws.w1t2 and b1t2 is ws.b1t2 and s1aT is W.s1aT
    gterm = seen["g3"][:, : W.F].double() @ W.s1bT.double()  # g3 s1g^T, the per-cloud part of both bias rows
    wd64 = w1t2.double() @ s1aT.double()
    bd64 = b1t2.double() @ s1aT.double() + W.s1b.double()
    tail = [(w.double(), b.double()) for w, b in l_layers[2:]]
    forms = {"layered": ([(w1t2.double(), b1t2.double()), (s1aT.double(), gterm + W.s1b.double())] + tail, l_relus),
             "collapsed": ([(wd64, gterm + bd64)] + tail, c_relus)}
    x = torch.cat((p, c), dim=2).double().as_subclass(_F64)
    out = {}
    for name, (layers, relus) in forms.items():
        o = torch.empty((B, N, W.C1), dtype=torch.float64)
        ph._chain_torch(x, N, 12, layers, relus, 1, out=o, out_cols=W.C1)
        out[name] = o
    err = (out["layered"] - out["collapsed"]).abs().max().item()
    scale = out["layered"].abs().max().item()
    print(f"collapsed vs layered chain D in float64 {err:.3e} (|log-prob| <= {scale:.3g})")
    assert torch.isfinite(out["layered"]).all() and err <= 1e-12 * max(scale, 1.0)
    # what the emulation's glue composed in fp32: 64 products per element, each factor rounded once
    e_w = (ws.wdT.double() - wd64).abs().max().item()
    e_b = (ws.bd.double() - bd64).abs().max().item()
    lim_w = 66 * 2.0 ** -24 * (w1t2.double().abs() @ s1aT.double().abs()).max().item()
    lim_b = 67 * 2.0 ** -24 * ((b1t2.double().abs() @ s1aT.double().abs()) + W.s1b.double().abs()).max().item()
    print(f"fp32 composition off by {e_w:.3e} (<= {lim_w:.3e}), bias {e_b:.3e} (<= {lim_b:.3e})")
    assert e_w <= lim_w and e_b <= lim_b
    # and the bias row the emulated forward gave chain D is the collapsed one
    e_c = (ws.cvec.double() - (gterm + bd64)).abs().max().item()
    lim_c = (67 + W.F + 2) * 2.0 ** -24 * ((seen["g3"][:, : W.F].double().abs() @ W.s1bT.double().abs())
                                            + (b1t2.double().abs() @ s1aT.double().abs())
                                            + W.s1b.double().abs()).max().item()
    print(f"fp32 bias row off by {e_c:.3e} (<= {lim_c:.3e})")
    assert e_c <= lim_c


@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_emulated_forwards_agree(monkeypatch, kind):
    """Collapsed and layered emulations (fp32 torch ops) against each other and torch's own composition."""
    from ndnet.models import pointnet_hip as ph
    monkeypatch.setattr(ph, "PRECISION", "x6")
    p, c = _inputs()
    outs = {}
    for collapse in (True, False):
        monkeypatch.setattr(ph, "COLLAPSE", collapse)
        m = _model(kind)
        outs[collapse] = _forward(ph, kind, m, p, c)
        (ws,) = m._hip["ws"].values()
        assert ws.collapses_b() == collapse and len(ws.specs[1][1]) == (3 if collapse else 4)
    with torch.no_grad():
        ref = m.forward_torch(p, c)
    d = (outs[True] - outs[False]).abs().max().item()
    print(f"{kind}: collapsed vs layered emulation {d:.3e}; vs torch {(outs[True] - ref).abs().max().item():.3e}")
    assert d < 1e-4 and (outs[True] - ref).abs().max().item() < 1e-4 and (outs[False] - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize("mode", ["fp32", "x3", "bf16"])
def test_other_modes_keep_the_layered_specs(monkeypatch, mode):
    from ndnet.models import pointnet_hip as ph
    monkeypatch.setattr(ph, "COLLAPSE", True)
    m = _model("seg")
    m.precision = mode
    p, c = _inputs()
    _forward(ph, "seg", m, p, c)
    (ws,) = m._hip["ws"].values()
    assert not ws.collapses_b() and not ws.collapses_d() and ws.specs is ws._specs[(False, False)]
    assert len(ws.specs[1][1]) == 4 and len(ws.specs[3][1]) == 5


# ---- the new fields' argument rules (include/ndnet_pointnet.h) ----

BUILDS = ("ndnet_pn_chain_run", "ndnet_pn_chain_run_t32")


def _block(edit):
    """A valid chain-B-like block over host memory (head prologue, 16 -> 64 per cloud on the VALU, 64 -> 128
    pooled), with the shared fold matrix and its bias attached, changed by `edit(ch, t)`."""
    from ndnet import _lib
    from ndnet.models import pointnet_hip as ph
    shapes = dict(w0=(2, 1024), b0=(64,), w1=(64 * 128,), b1=(128,), x=(2, 5, 12), gmax=(2, 128), h2=(2, 256),
                  w3=(9, 256), b3=(9,), basis=(9, 12 * 64), t1=(2, 9), m=(64, 64), mb=(64,))
    t = {k: torch.zeros(*s) for k, s in shapes.items()}
    ch = ph._build_chain(5, 12, [(t["w0"], 1024, t["b0"], 16, 64), (t["w1"], 0, t["b1"], 64, 128)], [1, 1], 0,
                         gmax=t["gmax"])
    ch.x = t["x"].data_ptr()
    ch.head_h2, ch.head_ld, ch.head_K = t["h2"].data_ptr(), 256, 256
    ch.head_w3, ch.head_b3, ch.head_basis = t["w3"].data_ptr(), t["b3"].data_ptr(), t["basis"].data_ptr()
    ch.head_kin, ch.head_nout, ch.head_t1 = 12, 64, t["t1"].data_ptr()
    ch.fold_t2, ch.fold_ld, ch.fold_bias, ch.x_nonfinite_nan = t["m"].data_ptr(), 0, t["mb"].data_ptr(), 1
    edit(ch, t)
    return [getattr(_lib.lib(), e)(ctypes.byref(ch), 2, None) for e in BUILDS]


def _mfma_layer0(ch, t):  # a one-layer chain runs layer 0 on the MFMA path: no fold, no flag there
    ch.num_layers = 1


COLLAPSE_ARG_CASES = {
    "fold_bias without fold_t2": lambda ch, t: setattr(ch, "fold_t2", None),
    "0 < fold_ld < 4096": lambda ch, t: setattr(ch, "fold_ld", 4092),
    "fold_ld % 4": lambda ch, t: setattr(ch, "fold_ld", 4098),
    "fold_t2 misaligned": lambda ch, t: setattr(ch, "fold_t2", t["m"].data_ptr() + 4),
    "x_nonfinite_nan = 2": lambda ch, t: setattr(ch, "x_nonfinite_nan", 2),
    "x_nonfinite_nan = -1": lambda ch, t: setattr(ch, "x_nonfinite_nan", -1),
    "layer 0 on the MFMA path": _mfma_layer0,
}


@pytest.mark.parametrize("case", sorted(COLLAPSE_ARG_CASES))
def test_inconsistent_collapse_blocks_are_rejected(case, capfd):
    """NDNET_ERR_ARG (-20) from both entry points, before anything is launched."""
    assert _block(COLLAPSE_ARG_CASES[case]) == [-20, -20]
    assert capfd.readouterr().err.count("invalid argument") == 2


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndnet_pointnet.h")


def _header_fields(struct, nested):
    """[(name, ctypes type)] of `typedef struct <struct> { ... } <struct>;` as include/ndnet_pointnet.h declares it."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", f.read()), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), text, re.S).group(1)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(\w+)\s+(\d+)\s*$", text, re.M)}
    scalars = dict(int32_t=ctypes.c_int32, int64_t=ctypes.c_int64, float=ctypes.c_float, **nested)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.fullmatch(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl, re.S).groups()
        base = scalars[ctype.replace("const", "").replace("*", "").strip()]
        for name in (n.strip() for n in names.split(",")):
            arr = re.fullmatch(r"(\w+)\[(\w+)\]", name)
            if "*" in ctype:
                fields.append((name, ctypes.c_void_p))
            elif arr:
                fields.append((arr.group(1), base * consts[arr.group(2)]))
            else:
                fields.append((name, base))
    return fields


def test_ctypes_mirror_matches_the_header():
    """``_Layer`` and ``_Chain`` field for field against the header's structs (names, order, types: a
    pointer is a c_void_p here); the appended fields sit at the end, after fold_out_b, 8-byte aligned."""
    from ndnet.models import pointnet_hip as ph
    layer = _header_fields("ndnet_pn_layer", {})
    assert layer == list(ph._Layer._fields_)
    chain = _header_fields("ndnet_pn_chain", dict(ndnet_pn_layer=ph._Layer))
    assert [n for n, _ in chain] == [f[0] for f in ph._Chain._fields_]
    for (name, want), (_, got) in zip(chain, ph._Chain._fields_):
        assert ctypes.sizeof(want) == ctypes.sizeof(got) and (want is got or name == "L"), name
    assert ph._Chain.L.size == ctypes.sizeof(ph._Layer) * ph.MAX_LAYERS
    names = [f[0] for f in ph._Chain._fields_]
    assert names[-4:] == ["fold_out_b", "fold_bias", "x_nonfinite_nan", "reserved0"]
    assert ph._Chain.fold_bias.offset == ph._Chain.fold_out_b.offset + 8
    assert ctypes.sizeof(ph._Chain) == ph._Chain.fold_bias.offset + 16
