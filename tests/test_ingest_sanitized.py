"""The native PLY reader under sanitizers, as a stand-alone program: tests/ingest_main.cpp and
ndt-net_amd/csrc/ply_ingest.cpp are compiled together, once with AddressSanitizer + UBSan and once
with ThreadSanitizer, and run as child processes over every file of tests/ingest_cases.py (the
corpus and the files that place the cuts of the parallel read) at 1 and 6 threads.  Each run has
to exit 0 without a sanitizer report and print what the plain library returns for the same call.

Nothing is loaded into Python and nothing is preloaded: the programs link their sanitizer's
runtime themselves.  Host code on the build machine: where a GPU is visible the test skips, and
without one it skips only if the compiler cannot link a one-line program with the sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import REPO, gpu_available

import ingest_cases as C

SRC = [os.path.join(REPO, "tests", "ingest_main.cpp"), os.path.join(REPO, "ndt-net_amd", "csrc", "ply_ingest.cpp")]
SANITIZERS = {"asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
              "tsan": ["-fsanitize=thread"]}
THREADS = (1, 6)
PROCESSES = 4  # each program runs its calls in four child processes side by side
MUL = 0x9E3779B97F4A7C15


def _cxx():
    return os.environ.get("CXX") or "g++"


def _hash(words):
    """ingest_main.cpp's hash_add over an array of unsigned integers, modulo 2^64."""
    w = np.ascontiguousarray(words).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((w ^ (w >> np.uint64(31))) * ((np.uint64(2) * i + np.uint64(1)) * np.uint64(MUL))).sum(
            dtype=np.uint64))


def _plain(path, header_lines, num_classes, threads):
    """The driver's output line for one call, from the plain library."""
    from ndnet import _lib
    lib = _lib.lib()
    bpath = os.fsencode(str(path))
    count = ctypes.c_uint64(0)
    crc = lib.ndnet_ply_count(bpath, header_lines, ctypes.byref(count))
    cap = count.value if crc == 0 else 0
    xyz = np.zeros((cap + 1, 3))
    cls = np.zeros(cap + 1, np.uint16)
    n = ctypes.c_uint64(0)
    rc = lib.ndnet_ply_read(bpath, header_lines, num_classes, xyz.ctypes.data, cls.ctypes.data, cap, ctypes.byref(n),
                            threads)
    got = n.value if rc == 0 else 0
    return (f"{crc} {cap} {rc} {n.value} {_hash(xyz[:got].view(np.uint64).ravel()):016x} "
            f"{_hash(cls[:got]):016x}")


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    """Every file written once; ``(list files, expected output lines)`` of all the calls."""
    if gpu_available():
        pytest.skip("sanitizers run on the build machine only, not where a GPU is visible")
    d = tmp_path_factory.mktemp("ingest_files")
    files = [(c.raw, c.header_lines, c.num_classes) for c in C.all_cases()] + list(C.structure_files().values())
    lines, expected = [], []
    for k, (raw, hl, nc) in enumerate(files):
        p = d / f"{k}.ply"
        p.write_bytes(raw)
        for th in THREADS:
            lines.append(f"{hl} {nc} {th} -1 {p}")
            expected.append(_plain(p, hl, nc, th))
    for extra in (f"{C.HL} {C.NC} 6 5 {d / '0.ply'}", f"{C.HL} {C.NC} 1 0 {d / '0.ply'}",  # more room; ERR_CAP
                  f"{C.HL} {C.NC} 6 -1 {d / 'missing.ply'}", f"{C.HL} {C.NC} 6 -1 {d}"):  # ERR_IO twice
        lines.append(extra)
    hl, nc = files[0][1], files[0][2]
    n0 = _plain(d / "0.ply", hl, nc, 1).split()
    expected += [" ".join(n0), f"0 {n0[1]} {C.ERR_CAP} {n0[1]} {0:016x} {0:016x}"]
    expected += [f"{C.ERR_IO} 0 {C.ERR_IO} 0 {0:016x} {0:016x}"] * 2
    listings = []
    for k in range(PROCESSES):  # call i is line i // PROCESSES of list i % PROCESSES
        listings.append(d / f"calls_{k}.txt")
        listings[-1].write_text("\n".join(lines[k::PROCESSES]) + "\n")
    return listings, expected


def _links(flags, tmp):
    one = tmp / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    return subprocess.run([_cxx(), *flags, "-o", str(tmp / "one"), str(one)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """Both sanitized programs, compiled side by side: ``{name: path, or None where the compiler
    cannot link the sanitizer at all}``."""
    if gpu_available():
        pytest.skip("sanitizers run on the build machine only, not where a GPU is visible")
    tmp = tmp_path_factory.mktemp("ingest_sanitized")
    jobs = {}
    for name, flags in SANITIZERS.items():
        out = tmp / f"ingest_main_{name}"
        cmd = [_cxx(), "-std=c++17", "-O1", "-g1", "-fno-omit-frame-pointer", "-Wall", *flags, "-o", str(out), *SRC,
               "-lpthread"]
        jobs[name] = (out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built = {}
    for name, (out, proc) in jobs.items():
        log = proc.communicate()[0]
        if proc.returncode == 0:
            built[name] = out
        else:
            assert not _links(SANITIZERS[name], tmp), f"{name}: the sanitizer links, the driver does not build:\n{log}"
            built[name] = None
    return built


@pytest.mark.parametrize("name", sorted(SANITIZERS))
def test_reader_under_sanitizer(name, programs, calls):
    if programs[name] is None:
        pytest.skip(f"{_cxx()} cannot link a program with {' '.join(SANITIZERS[name])}")
    listings, expected = calls
    runs = [subprocess.Popen([str(programs[name]), "@" + str(ls)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True) for ls in listings]
    got = [None] * len(expected)
    for k, run in enumerate(runs):
        out, err = run.communicate()
        assert err == "", err[-4000:]
        assert run.returncode == 0
        part = out.splitlines()
        assert len(part) == len(got[k::PROCESSES])
        got[k::PROCESSES] = part
    wrong = [(k, g, e) for k, (g, e) in enumerate(zip(got, expected)) if g != e]
    assert not wrong, wrong[:5]
    assert sum(e.split()[2] == "0" for e in expected) > 400 and sum(e.split()[2] != "0" for e in expected) > 400


def test_driver_single_call(programs, calls, tmp_path):
    """The one-call form of the driver's command line gives the list form's line."""
    name = next((k for k, v in sorted(programs.items()) if v), None)
    if name is None:
        pytest.skip(f"{_cxx()} cannot link a program with a sanitizer")
    raw, hl, nc = C.structure_files()["just_over_64k"]
    p = tmp_path / "one.ply"
    p.write_bytes(raw)
    run = subprocess.run([str(programs[name]), str(p), str(hl), str(nc), "2"], capture_output=True, text=True)
    assert (run.returncode, run.stderr) == (0, "")
    assert run.stdout.strip() == _plain(p, hl, nc, 2)
