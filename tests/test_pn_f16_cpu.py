"""The fp16 two-slice form without a GPU: the host restatement of its weight fold (``_frag_f16``), the
argument rules of ndnet_pn_chain_f16_run and ndnet_pn_fold16_check on host memory (both return before
anything is launched), the ctypes mirrors against include/ndnet_pointnet.h, and the switch."""
import ctypes
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndnet_pointnet.h")
MAKEFILE = os.path.join(os.path.dirname(HEADER), "..", "ndt-net_amd", "Makefile")


def _ph():
    from ndnet.models import pointnet_hip as ph
    return ph


def _unfrag16(planes, K, N):
    """[2][K][N] from the flattened [cb][kg][plane][kq][cl][j] layout (k = 32 kg + 8 kq + j, n = 16 cb + cl)."""
    v = planes.reshape(N // 16, K // 32, 2, 4, 16, 8)  # cb, kg, plane, kq, cl, j
    return v.permute(2, 1, 3, 5, 0, 4).reshape(2, K, N)


@pytest.mark.parametrize("K,N,mag", [(64, 128, 0.3), (128, 1024, 1e-3), (512, 256, 40.0), (32, 16, 1e-20)])
def test_two_slices_carry_the_scaled_weight(K, N, mag):
    """h + l against w 2^s: the scale is a power of two that puts the maximum in [2^13, 2^14); h is the
    nearest fp16 and l the nearest fp16 of the exact residual, so the pair is within 2^-23 of every element
    at or above 2^-10 (where l is a normal fp16 or the residual is exact) and within 2^-25 absolutely below."""
    ph = _ph()
    g = torch.Generator().manual_seed(K + N)
    w = torch.randn(K, N, generator=g) * mag
    planes, scale = ph._frag_f16(w)
    assert planes.dtype == torch.float16 and planes.numel() == 2 * K * N and scale.shape == (1,)
    inv = float(scale)
    s = -round(torch.log2(scale).item())
    assert inv == 2.0 ** -s
    top = float(w.abs().max()) * 2.0 ** s
    assert 2.0 ** 13 <= top < 2.0 ** 14
    h, lo = _unfrag16(planes, K, N).double()
    x = w.double() * 2.0 ** s
    assert torch.equal(h.float().half(), (w * 2.0 ** s).half()) and torch.isfinite(h).all()
    err = (h + lo - x).abs()
    assert bool((err <= torch.maximum(x.abs() * 2.0 ** -23, torch.full_like(x, 2.0 ** -25))).all())
    assert bool((lo.abs() <= h.abs() * 2.0 ** -11 + 2.0 ** -25).all())


def test_layout_is_the_split_bf16_one_with_two_planes():
    ph = _ph()
    K, N = 64, 32
    w = (torch.arange(K * N, dtype=torch.float32).reshape(K, N) + 1) / 4  # exact in fp16 after the scale: l = 0
    planes, scale = ph._frag_f16(w)
    s = -round(torch.log2(scale).item())
    for k, n in [(0, 0), (7, 15), (8, 0), (31, 16), (32, 1), (63, 31)]:
        cb, cl, kg, kq, j = n // 16, n % 16, k // 32, (k % 32) // 8, k % 8
        at = ((((cb * (K // 32) + kg) * 2 + 0) * 4 + kq) * 16 + cl) * 8 + j
        assert float(planes[at]) == float(w[k, n]) * 2.0 ** s and float(planes[at + 4 * 16 * 8]) == 0.0
    x6 = ph._frag_x6(w).reshape(N // 16, K // 32, 3, 4, 16, 8)
    assert planes.reshape(N // 16, K // 32, 2, 4, 16, 8).shape[3:] == x6.shape[3:]


def test_degenerate_layers():
    ph = _ph()
    planes, scale = ph._frag_f16(torch.zeros(32, 16))
    assert float(scale) == 1.0 and not bool(planes.any())
    w = torch.zeros(32, 16)
    w[1, 2] = 0.5
    planes, scale = ph._frag_f16(w)
    assert float(scale) == 2.0 ** -14 and float(planes.float().abs().max()) == 2.0 ** 13
    w[1, 2] = 2.0 ** -140  # a subnormal maximum: the exponent stops at 100, the planes stay small
    assert float(ph._frag_f16(w)[1]) == 2.0 ** -100
    w[1, 2] = 2.0 ** 127   # the largest exponent: s = -114, the maximum lands at 2^13 and nothing overflows
    planes, scale = ph._frag_f16(w)
    assert float(scale) == 2.0 ** 114 and float(planes.float().abs().max()) == 2.0 ** 13
    assert ph._f16_exponent(3.0e38) == -114 and ph._f16_exponent(2.0 ** -149) == 100
    assert ph._f16_exponent(float("inf")) == 0 and ph._f16_exponent(float("nan")) == 0 and ph._f16_exponent(0.0) == 0
    assert ph._f16_exponent(1.0) == 13 and ph._f16_exponent(1.999) == 13 and ph._f16_exponent(2.0) == 12


def test_folded_model_has_a_job_per_split_layer():
    """The fp16 planes sit beside the bf16 ones, their recipes in a list of their own (``jobs`` is unchanged)."""
    from model_init import deterministic_state
    from ndnet.models.ndtnet import NDTNetSegmentation
    from ndnet.models.pointnet import PointNetSegmentation
    ph = _ph()
    m = NDTNetSegmentation(3, 5, 64)
    m.load_state_dict(deterministic_state(m.state_dict()))
    W = ph._Folded(m.eval())
    assert W.frag16 == {} and W.jobs16 == [], "nothing of the fp16 form before a forward takes it"
    assert W.ensure_f16() and W.ensure_f16()
    assert set(W.frag16) == set(W.frag6) == {id(w) for w in W.wide} and len(W.jobs16) == len(W.wide)
    assert all(j[0] <= 5 for j in W.jobs)
    for w in W.wide:
        planes, scale = ph._frag_f16(w)
        assert torch.equal(W.frag16[id(w)].view(torch.int16), planes.view(torch.int16)) and torch.equal(W.scale16[id(w)], scale)
        assert W.frag16[id(w)].numel() * 3 == W.frag6[id(w)].numel() * 2
    for (out, part, scale, layer, bn, k0, K, Kp, Np), w in zip(W.jobs16, W.wide):
        assert out is W.frag16[id(w)] and scale is W.scale16[id(w)] and part.numel() == 16 and (Kp, Np) == tuple(w.shape)
    b = PointNetSegmentation(3, 5, 64)
    b.load_state_dict(deterministic_state(b.state_dict()))
    Wb = ph._Folded(b.eval())
    assert not Wb.ensure_f16() and Wb.frag16 == {} and Wb.jobs16 == []


def test_slices_switch():
    ph = _ph()
    assert ph.SLICES == os.environ.get("NDNET_PN_SLICES", "f16")
    assert ph._slices("f16") == "f16" and ph._slices("bf16") == "bf16"
    for bad in ("fp8", "", "F16", "x6"):
        with pytest.raises(ValueError):
            ph._slices(bad)


# ---- argument rules, on host memory: every case returns before a launch ----

BUILDS = ("ndnet_pn_chain_f16_run", "ndnet_pn_chain_f16_run_t32")


def _block(edit):
    """A chain-A-like block over host memory (16 -> 64 on the VALU, 64 -> 128, 128 -> 256 pooled, both split)
    with its fp16 block, made invalid by `edit(ch, ext, t)`."""
    from ndnet import _lib
    ph = _ph()
    shapes = dict(w0=(1024,), b0=(64,), w1=(64 * 128 * 3 // 2,), b1=(128,), w2=(128 * 256 * 3 // 2,), b2=(256,),
                  x=(2, 5, 12), gmax=(2, 256), p1=(64 * 128,), p2=(128 * 256,), s=(2,), n=(1,))
    t = {k: torch.zeros(*s) for k, s in shapes.items()}
    ch = ph._build_chain(5, 3, [(t["w0"], 0, t["b0"], 16, 64), (t["w1"], 0, t["b1"], 64, 128, 1),
                                (t["w2"], 0, t["b2"], 128, 256, 1)], [1, 1, 1], 0, gmax=t["gmax"])
    ch.x = t["x"].data_ptr()
    ext = ph._F16()
    ext.w16[1], ext.w16[2] = t["p1"].data_ptr(), t["p2"].data_ptr()
    ext.scale[1], ext.scale[2] = t["s"].data_ptr(), t["s"].data_ptr() + 4
    ext.fallbacks = t["n"].data_ptr()
    ext_arg = edit(ch, ext, t)
    ext_arg = ctypes.byref(ext) if ext_arg is None else ext_arg
    return [getattr(_lib.lib(), e)(ctypes.byref(ch), None if ext_arg == "null" else ext_arg, 2, None) for e in BUILDS]


def _set_item(field, i, value):
    def edit(ch, ext, t):
        getattr(ext, field)[i] = value
    return edit


def _layer_field(l, field, value):
    def edit(ch, ext, t):
        setattr(ch.L[l], field, value)
    return edit


def _no_split_layer(ch, ext, t):
    ch.num_layers = 1
    ch.max_width2 = 64


def _pooled_q(ch, ext, t):  # 64 -> 128 produced in chunks straight into the pooled 128 -> 256
    ch.L[1].fuse_next = 1


def _fused_split_p(ch, ext, t):  # a log-softmax chain, so only the split layer's fuse_next is at fault
    ch.L[1].fuse_next = 1
    ch.mode, ch.out_cols, ch.out = 1, 29, t["gmax"].data_ptr()


F16_ARG_CASES = {
    "no fp16 block": lambda ch, ext, t: "null",
    "no counter": lambda ch, ext, t: setattr(ext, "fallbacks", None),
    "a split layer without planes": _set_item("w16", 2, None),
    "a split layer without a scale": _set_item("scale", 1, None),
    "planes misaligned": lambda ch, ext, t: _set_item("w16", 1, t["p1"].data_ptr() + 8)(ch, ext, t),
    "prec 2": lambda ch, ext, t: (_layer_field(1, "prec", 2)(ch, ext, t), _layer_field(2, "prec", 2)(ch, ext, t))[0],
    "prec 3": lambda ch, ext, t: (_layer_field(1, "prec", 3)(ch, ext, t), _layer_field(2, "prec", 3)(ch, ext, t))[0],
    "prec 4": _layer_field(2, "prec", 4),
    "per-cloud split weights": _layer_field(1, "w_cloud_stride", 64 * 128 * 3 // 2),
    "no split layer": _no_split_layer,
    "a pooled last layer fed by a fused one": _pooled_q,
    "a split layer fused into the next": _fused_split_p,
}


@pytest.mark.parametrize("case", sorted(F16_ARG_CASES))
def test_inconsistent_f16_blocks_are_rejected(case, capfd):
    """NDNET_ERR_ARG (-20) from both entry points, before anything is launched."""
    assert _block(F16_ARG_CASES[case]) == [-20, -20]
    assert capfd.readouterr().err.count("invalid argument") == 2


def _job(**edit):
    ph = _ph()
    t = dict(w=torch.zeros(100, 70), out=torch.zeros(64 * 128 * 2, dtype=torch.float16), part=torch.zeros(16),
             scale=torch.zeros(1), g=torch.ones(100), v=torch.ones(100))
    J = ph._Fold16Job()
    J.w, J.out, J.partial, J.scale = (t[k].data_ptr() for k in ("w", "out", "part", "scale"))
    J.gamma, J.var, J.eps = t["g"].data_ptr(), t["v"].data_ptr(), 1e-5
    J.N, J.K, J.ld, J.k0, J.Kp, J.Np = 100, 64, 70, 6, 64, 128
    for k, v in edit.items():
        setattr(J, k, v(t) if callable(v) else v)
    return J, t


def test_fold16_check_on_host_memory():
    from ndnet import _lib
    check = _lib.lib().ndnet_pn_fold16_check
    units = ctypes.c_int64(-1)
    J, keep = _job()
    assert check(ctypes.byref(J), 1, ctypes.byref(units)) == 0 and units.value == 64 * 128 // 8
    assert check(None, 1, ctypes.byref(units)) == -20 and check(ctypes.byref(J), 0, ctypes.byref(units)) == -20
    assert check(ctypes.byref(J), 1, None) == -20
    bad = [dict(w=None), dict(out=None), dict(partial=None), dict(scale=None), dict(out=lambda t: t["out"].data_ptr() + 8),
           dict(N=0), dict(K=0), dict(k0=-1), dict(ld=69), dict(Kp=32), dict(Np=96), dict(Kp=80), dict(Np=136),
           dict(gamma=None), dict(var=None), dict(eps=-1.0)]
    for edit in bad:
        J, keep = _job(**edit)
        assert check(ctypes.byref(J), 1, ctypes.byref(units)) == -20, edit
    J, keep = _job(gamma=None, var=None)  # no BatchNorm at all is a valid job
    assert check(ctypes.byref(J), 1, ctypes.byref(units)) == 0
    run = _lib.lib().ndnet_pn_fold16_run
    assert run(None, 1, 1024, None) == -20 and run(ctypes.byref(J), 0, 1024, None) == -20
    assert run(ctypes.byref(J), 1, 0, None) == -20
    assert _lib.lib().ndnet_pn_take_f16_fallbacks(None, None) == -20


# ---- the ctypes mirrors against the header ----

_SCALARS = dict(int32_t=ctypes.c_int32, int64_t=ctypes.c_int64, float=ctypes.c_float, uint32_t=ctypes.c_uint32)


def _struct_fields(name):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", f.read()), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, re.S).group(1)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(\w+)\s+(\d+)\s*$", text, re.M)}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.fullmatch(r"((?:const\s+)?\w+)\s*(.*)", decl, re.S).groups()
        for n in (n.strip() for n in names.split(",")):
            ptr = n.startswith("*")
            n = n.lstrip("* ")
            base = ctypes.c_void_p if ptr else _SCALARS[ctype.replace("const", "").strip()]
            arr = re.fullmatch(r"(\w+)\[(\w+)\]", n)
            fields.append((arr.group(1), base * consts[arr.group(2)]) if arr else (n, base))
    return fields


@pytest.mark.parametrize("struct,mirror", [("ndnet_pn_f16", "_F16"), ("ndnet_pn_fold16_job", "_Fold16Job")])
def test_new_mirrors_match_the_header(struct, mirror):
    want, got = _struct_fields(struct), list(getattr(_ph(), mirror)._fields_)
    assert [n for n, _ in want] == [n for n, _ in got]
    for (n, a), (_, b) in zip(want, got):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is b or hasattr(a, "_length_")), n
    assert ctypes.sizeof(_ph()._F16) == 8 * (2 * _ph().MAX_LAYERS + 1)


def test_released_structs_keep_their_size():
    """The fp16 form travels in a block of its own: ndnet_pn_chain, ndnet_pn_layer and ndnet_pn_fold_job end
    where they ended (tests/test_collapse_cpu.py and tests/test_fold_products_cpu.py pin their last fields)."""
    ph = _ph()
    assert [f[0] for f in ph._Chain._fields_][-1] == "reserved0" and [f[0] for f in ph._FoldJob._fields_][-1] == "reserved1"
    assert [f[0] for f in ph._Layer._fields_][-1] == "fuse_next"


def test_no_flush_flag_in_the_build():
    """The window's lower edge relies on the f16 MFMA keeping subnormal inputs: nothing in the build may
    switch the kernels to flush them."""
    with open(MAKEFILE) as f:
        text = f.read()
    for flag in ("denormals-are-zero", "ftz", "daz", "fp32-denormals", "denormal-fp-math", "fast-math=", "-ffast-math", "-Ofast"):
        assert flag not in text.replace("-fno-fast-math", ""), flag
