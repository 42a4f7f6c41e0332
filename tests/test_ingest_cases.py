"""The native ASCII-PLY reader (ndt-net_amd/csrc/ply_ingest.cpp) against the reference's Python
loop (oracle/ingest_oracle.py) on the files of tests/ingest_cases.py, under the rule of
include/ndnet_ingest.h:

  both read        the same number of points; xyz equal bit for bit (NaN by position, the sign of
                   zero included); the class tags equal;
  oracle reads,    only for the header's closed "stricter than the reference" list: the listed
  reader refuses   error code, and *n_out = the 0-based index of the refused data line;
  oracle raises    the reader fails too (blank lines apart, which it skips): NDNET_PLY_ERR_CLASS
                   where the oracle's error is the class bound, NDNET_PLY_ERR_PARSE otherwise,
                   at the same data line.

and the structure of the parallel read: the result at every number of threads is the
one-thread result, wherever the cuts between the ranges fall.  Host code: runs on the CPU."""
import ctypes
import os

import numpy as np
import pytest

import ingest_cases as C

NAMED = C.number_cases() + C.tag_cases() + C.structure_cases()


def _write(tmp_path, name, raw):
    p = tmp_path / name
    p.write_bytes(raw)
    return p


def _check(case, path, threads=1):
    """None, or what is wrong with the reader's answer for ``case``."""
    exp = C.expected(case)
    got = C.native_read(path, case.header_lines, case.num_classes, threads)
    if not got.untouched:
        return f"{case.name}: wrote outside the rows it may write"
    if exp[0] == C.OK:
        if got.rc != C.OK:
            return f"{case.name} ({case.kind}): rc {got.rc} at line {got.n}, the oracle reads {len(exp[2])} points"
        if got.n != len(exp[2]):
            return f"{case.name}: {got.n} points, the oracle {len(exp[2])}"
        if not C.same_bits(got.xyz, exp[1]):
            bad = np.argwhere(got.xyz.view(np.uint64) != exp[1].view(np.uint64))[:3].tolist()
            return f"{case.name}: xyz differs at {bad}: {got.xyz[bad[0][0]]} for {exp[1][bad[0][0]]}"
        if not np.array_equal(got.cls, exp[2]):
            return f"{case.name}: class tags differ"
        rc, count = C.native_count(path, case.header_lines)
        if (rc, count) != (C.OK, got.n):
            return f"{case.name}: ndnet_ply_count gives rc {rc}, {count} for {got.n} points"
        return None
    code, index = exp
    if got.rc != code:
        return f"{case.name} ({case.kind}): rc {got.rc} (n {got.n}) for {code}"
    if index is not None and got.n != index:
        return f"{case.name} ({case.kind}): reports data line {got.n} for {index}"
    return None


def test_stricter_list_is_the_headers():
    """The header's closed list and the corpus's are one list, and each entry has a case."""
    assert C.header_stricter() == C.STRICTER
    used = {c.why for c in C.all_cases() if c.kind == "stricter"}
    assert used == set(C.STRICTER)


def test_corpus_kinds():
    """The kinds come from the oracle; the rows that started this corpus have the kind they had."""
    by = {c.name: c for c in NAMED}
    assert len(by) == len(NAMED)
    for name, kind in {"line[lone_cr]": "same", "num[1e999]": "same", "num[-1e999]": "same",
                       "num[1e-999]": "same", "num[-1e-999]": "same", "num[nan(1)]": "both_fail",
                       "num[+nan(1)]": "both_fail", "num[+-1]": "both_fail", "num[++1]": "both_fail",
                       "tag[99999999999999999999]": "both_fail", "tag[-99999999999999999999]": "stricter",
                       "tag[65535]": "both_fail", "tag_bound[65535,nc=65535]": "same", "tag[+4]": "same",
                       "tag[-0]": "same", "tag[4.0]": "both_fail", "tag[1_0]": "stricter", "tag[-1]": "stricter",
                       "line[three_tokens]": "stricter", "line[blank_middle]": "same", "line[empty_file]": "same",
                       "line[header_longer_than_file]": "same", "line[nul_in_x]": "both_fail",
                       "line[not_utf8_in_z]": "not_utf8", "line[not_utf8_in_header]": "not_utf8",
                       "line[not_utf8_unread_column]": "not_utf8", "num[1_0]": "stricter", "num[inf]": "same",
                       "num[-nan]": "same", "num[1e]": "both_fail", "num[0x10]": "both_fail"}.items():
        assert by[name].kind == kind, (name, by[name].kind)
    for c in NAMED:  # a reason goes with a stricter case; the two that are not stand in the header
        assert (c.kind == "stricter") == (c.why is not None) or c.name in (
            "line[space_00a0_class]", "line[unicode_digit_class]"), c.name
    # 1e999 overflows and 1e-999 underflows in the oracle as the issue's table says
    assert C.expected(by["num[-1e999]"])[1][1].min() == -np.inf
    row = C.expected(by["num[-1e-999]"])[1][1]
    assert ((row == 0) & np.signbit(row)).sum() == 1


def test_fuzz_shares():
    """About 2000 lines; the oracle alone puts at most a tenth of them on the stricter list, and
    neither the lines that read nor the lines that fail are a small minority."""
    f = C.fuzz()
    total = f.n_same + f.n_stricter + f.n_both_fail
    assert total == C.FUZZ_LINES == 2000
    print(f"fuzz: {f.n_same} same, {f.n_stricter} stricter ({f.n_stricter / total:.1%}), {f.n_both_fail} both_fail")
    assert 0 < f.n_stricter <= 0.10 * total
    assert f.n_same >= 0.25 * total and f.n_both_fail >= 0.15 * total
    assert {c.why for c in f.refused if c.why} == {"underscore", "few_tokens", "negative_tag"}
    assert all(C.stricter_reason(ln) is None for ln in f.accepted.raw[len(C.HEADER):].decode().split("\n") if ln)


@pytest.mark.parametrize("case", NAMED, ids=[c.name for c in NAMED])
def test_named_case(case, tmp_path):
    p = _write(tmp_path, "case.ply", case.raw)
    assert _check(case, p) is None


def test_fuzz_accepted_lines(tmp_path):
    f = C.fuzz()
    p = _write(tmp_path, "accepted.ply", f.accepted.raw)
    assert C.expected(f.accepted)[1].shape[0] == f.n_same
    for th in (1, 3):
        assert _check(f.accepted, p, th) is None


def test_fuzz_refused_lines(tmp_path):
    """Each line the oracle refuses, or reads and the list refuses, in a file of its own: the
    reader fails with the code and at the line the rule gives."""
    wrong = []
    for i, case in enumerate(C.fuzz().refused):
        msg = _check(case, _write(tmp_path, f"{i}.ply", case.raw))
        if msg:
            wrong.append(msg + " " + repr(case.raw[case.at:]))
    assert not wrong, f"{len(wrong)} of {len(C.fuzz().refused)}: " + "; ".join(wrong[:20])


# ---------------------------------------------------------------------------------------------
# the structure of the parallel read

@pytest.mark.parametrize("name", sorted(C.structure_files()))
def test_every_thread_count_gives_the_one_thread_result(name, tmp_path):
    raw, hl, nc = C.structure_files()[name]
    p = _write(tmp_path, name + ".ply", raw)
    one = C.native_read(p, hl, nc, 1)
    assert one.untouched
    exp = C.oracle(raw, hl, nc)
    if exp[0] == "ok":  # and the one-thread result is the oracle's
        assert one.rc == C.OK and C.same_bits(one.xyz, exp[1]) and np.array_equal(one.cls, exp[2])
        assert C.native_count(p, hl) == (C.OK, one.n)
    else:
        is_class = str(exp[1]).startswith("Class tag")
        assert (one.rc, one.n) == (C.ERR_CLASS if is_class else C.ERR_PARSE, exp[2])
    for th in C.THREADS[1:]:
        got = C.native_read(p, hl, nc, th)
        assert got.untouched, th
        assert (got.rc, got.n) == (one.rc, one.n), th
        assert got.xyz.tobytes() == one.xyz.tobytes() and got.cls.tobytes() == one.cls.tobytes(), th


def test_lone_cr_lines_read_in_linear_time(tmp_path):
    """4 MB of 16-byte lines ending in a lone '\\r', a file without one '\\n': the count, the read
    and a header skip of half the lines each take no more than ten times what they take for the
    same lines ending in '\\n', plus 0.2 s for the machine's noise (best of three).  The line ends
    cost the same search either way, so a linear reader is within a small factor; one that
    searches the rest of the file anew for each line does 262144 searches of 2 MB on average,
    minutes against milliseconds."""
    import time
    from ndnet import _lib
    lib = _lib.lib()
    cr = C.structure_files()["cr_lines_4mb"][0]
    paths = {"cr": _write(tmp_path, "cr.ply", cr), "lf": _write(tmp_path, "lf.ply", cr.replace(b"\r", b"\n"))}
    n = ctypes.c_uint64(0)
    xyz = np.empty((C.CR_LINES, 3))
    cls = np.empty(C.CR_LINES, np.uint16)

    def best(fn):
        times = []
        for _ in range(3):
            t = time.perf_counter()
            assert fn() == C.OK
            times.append(time.perf_counter() - t)
        return min(times)

    for what, hl in (("count", C.HL), ("read", C.HL), ("read", C.HL + C.CR_LINES // 2)):
        took = {}
        for end, p in paths.items():
            bp = os.fsencode(str(p))
            if what == "count":
                took[end] = best(lambda: lib.ndnet_ply_count(bp, hl, ctypes.byref(n)))
            else:
                took[end] = best(lambda: lib.ndnet_ply_read(bp, hl, C.NC, xyz.ctypes.data, cls.ctypes.data,
                                                            C.CR_LINES, ctypes.byref(n), 1))
            assert n.value == C.CR_LINES - (hl - C.HL)
        print(f"{what} after {hl} header lines: cr {took['cr'] * 1e3:.1f} ms, lf {took['lf'] * 1e3:.1f} ms")
        assert took["cr"] <= 10 * took["lf"] + 0.2, (what, hl, took)


def test_structure_files_are_what_they_claim():
    f = C.structure_files()
    raw = f["fixed64"][0]
    assert len(raw) >= 6 * C.CUT and all(raw[k * C.CUT - 1:k * C.CUT] == b"\n" for k in range(1, 7))
    assert all(f["fixed64_shifted"][0][k * C.CUT:k * C.CUT + 1] == b"\n" for k in range(1, 7))
    assert b"\n" not in f["fixed64_cr"][0] and f["fixed64_crlf"][0].count(b"\r\n") == len(raw) // 64
    assert max(len(ln) for ln in f["long_line"][0].split(b"\n")) > 300_000
    assert len(f["just_under_64k"][0]) == C.CUT - 1 and len(f["exactly_64k"][0]) == C.CUT
    for name, first in (("class_early_parse_late", "Class tag"), ("parse_early_class_late", "could not convert")):
        kind, exc, index = C.oracle(*f[name])
        assert kind == "raise" and str(exc).startswith(first) and index == C.EARLY
    assert C.EARLY * 64 < len(raw) // 6 and C.LATE * 64 > 5 * len(raw) // 6  # the first and the last of six ranges
    for name in ("class_late_only", "parse_late_only"):
        assert C.oracle(*f[name])[2] == C.LATE


# ---------------------------------------------------------------------------------------------
# arguments, capacity, Python errors

def _good_file(tmp_path, n=1000):
    raw = C.HEADER + b"".join(C._fixed_line(i) for i in range(n))
    return _write(tmp_path, "good.ply", raw), n


@pytest.mark.parametrize("short_by", ["one", "all"])
def test_capacity_error_writes_nothing(tmp_path, short_by):
    p, n = _good_file(tmp_path)
    cap = n - 1 if short_by == "one" else 0
    for th in (1, 4):
        got = C.native_read(p, C.HL, C.NC, th, capacity=cap)
        assert (got.rc, got.n) == (C.ERR_CAP, n)
        assert got.untouched  # for NDNET_PLY_ERR_CAP: not one row
    got = C.native_read(p, C.HL, C.NC, 2, capacity=n + 5)  # more room than points: the rest stays
    assert (got.rc, got.n) == (C.OK, n) and got.untouched


def test_argument_errors(tmp_path):
    from ndnet import _lib
    lib = _lib.lib()
    p, n = _good_file(tmp_path, 10)
    path = os.fsencode(str(p))
    xyz = np.zeros((n, 3))
    cls = np.zeros(n, np.uint16)
    out = ctypes.c_uint64(0)
    X, K, N = xyz.ctypes.data, cls.ctypes.data, ctypes.byref(out)
    assert lib.ndnet_ply_read(path, C.HL, C.NC, X, K, n, N, 1) == C.OK and out.value == n
    assert lib.ndnet_ply_read(None, C.HL, C.NC, X, K, n, N, 1) == C.ERR_ARG
    assert lib.ndnet_ply_read(path, C.HL, C.NC, None, K, n, N, 1) == C.ERR_ARG
    assert lib.ndnet_ply_read(path, C.HL, C.NC, X, None, n, N, 1) == C.ERR_ARG
    assert lib.ndnet_ply_read(path, C.HL, C.NC, X, K, n, None, 1) == C.ERR_ARG
    assert lib.ndnet_ply_read(path, -1, C.NC, X, K, n, N, 1) == C.ERR_ARG
    assert lib.ndnet_ply_count(None, C.HL, N) == C.ERR_ARG
    assert lib.ndnet_ply_count(path, C.HL, None) == C.ERR_ARG
    assert lib.ndnet_ply_count(path, -1, N) == C.ERR_ARG
    missing = os.fsencode(str(tmp_path / "missing.ply"))
    folder = os.fsencode(str(tmp_path))
    for bad in (missing, folder):
        assert lib.ndnet_ply_count(bad, C.HL, N) == C.ERR_IO
        assert lib.ndnet_ply_read(bad, C.HL, C.NC, X, K, n, N, 1) == C.ERR_IO


def test_num_classes_past_uint16_is_an_argument_error(tmp_path):
    """cls is uint16: with num_classes = 70000 a tag 65536 passes the reference's bound and would
    be stored as 0.  The reader refuses such a num_classes, and read_ply before it opens a file."""
    from ndnet.datasets.carla_seg import read_ply
    raw = C.HEADER + b"1 2 3 65536\n"
    assert C.oracle(raw, C.HL, 70000)[2] == [65536]
    p = _write(tmp_path, "wide.ply", raw)
    for nc in (65536, 70000, 2**31 - 1):
        got = C.native_read(p, C.HL, nc, 1, capacity=1)
        assert got.rc == C.ERR_ARG and got.untouched
        with pytest.raises(ValueError, match="num_classes"):
            read_ply(str(tmp_path / "missing.ply"), nc)
    got = C.native_read(p, C.HL, 65535, 1)
    assert (got.rc, got.n) == (C.ERR_CLASS, 0)


def test_python_errors_name_the_line(tmp_path):
    from ndnet.datasets import CARLA_Seg
    from ndnet.datasets.carla_seg import read_ply
    d = tmp_path / "scans"
    d.mkdir()
    good = b"".join(C._fixed_line(i) for i in range(40))
    (d / "0_class.ply").write_bytes(C.HEADER + good + b"\n\n1 2 3 99\n" + good)
    (d / "1_parse.ply").write_bytes(C.HEADER + good + good + b"1 2 nan(1) 4\n")
    (d / "2_ok.ply").write_bytes(C.HEADER + good)
    with pytest.raises(ValueError, match=r"Class tag out of bounds on data line 40 of .*0_class\.ply"):
        read_ply(str(d / "0_class.ply"), C.NC, C.HL)
    with pytest.raises(ValueError, match=r"Malformed data line 80 of .*1_parse\.ply"):
        read_ply(str(d / "1_parse.ply"), C.NC, C.HL, threads=3)
    with pytest.raises(FileNotFoundError):
        read_ply(str(d / "none.ply"), C.NC)
    with pytest.raises(FileNotFoundError):
        read_ply(str(d), C.NC)
    ds = CARLA_Seg(C.NC, None, str(d))
    with pytest.raises(ValueError, match="Class tag out of bounds on data line 40"):
        ds.get_data_pcl(str(d / "0_class.ply"), C.HL)
    with pytest.raises(ValueError, match="Malformed data line 80"):
        ds.get_data_pcl(str(d / "1_parse.ply"), C.HL)
    pts, cls = ds.get_data_pcl(str(d / "2_ok.ply"), C.HL)
    assert pts.shape == (40, 3) and cls.shape == (40,)
