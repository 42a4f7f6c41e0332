"""Named files for the native ASCII-PLY reader (include/ndnet_ingest.h) against the reference's
Python loop as oracle/ingest_oracle.py restates it (a helper of test_ingest_cases.py and
test_ingest_sanitized.py, not a conftest): every spelling of a number float() and int() take or
refuse, the class tag's bounds, the line endings and blanks, empty and header-only files, a
seeded grammar fuzz, and the files that put the cuts of the parallel read in chosen places.

A case is the file's bytes, ``num_header_lines``, ``num_classes`` and its kind:

``same``       the oracle reads the file and the reader returns the same points, bit for bit;
``stricter``   the oracle reads it and the reader refuses it, for a reason on the header's closed
               list (``why``, a key of ``STRICTER``), at the data line starting at byte ``at``;
``both_fail``  the oracle raises (blank lines apart, which both skip) and the reader fails;
``not_utf8``   the file does not decode, so the reference's open() fails it wherever the bytes
               stand; the reader decodes nothing and fails only where such bytes lie in a token
               that it reads.  It has to return what the oracle makes of the file opened with
               ``errors="surrogateescape"``, which keeps each such byte as a character that is
               neither a blank nor a digit (the header's second exception).

The kind is what the oracle does with the bytes (``_case`` runs it), and ``expected`` gives what
the reader has to return, from the oracle's parse alone: no expected value is a literal here.
Everything is built on import, in well under a second.
"""
import ctypes
import functools
import os
import random
import re
from collections import namedtuple

import numpy as np

import ingest_oracle as O

OK, ERR_ARG, ERR_IO, ERR_PARSE, ERR_CLASS, ERR_CAP = 0, -20, -30, -31, -32, -33
CODES = {"PARSE": ERR_PARSE, "CLASS": ERR_CLASS}

# The closed list of include/ndnet_ingest.h: what the reference reads and the reader refuses.
STRICTER = {
    "few_tokens": "PARSE",
    "negative_tag": "CLASS",
    "underscore": "PARSE",
    "other_space": "PARSE",
    "nul_byte": "PARSE",
    "unicode_digit": "PARSE",
}

NOT_DECODED = ("other_space", "unicode_digit")  # the reasons that lie in non-ASCII bytes
BLANKS = (" ", "\t", "\v", "\f")  # what the reader takes between tokens ('\r' ends a line)
THREADS = (1, 2, 3, 5, 6, 7, 64, 0, -5)
HEADER = b"ply\nformat ascii 1.0\nend_header\n"
HL = 3
NC = 28

Case = namedtuple("Case", "name raw header_lines num_classes kind why at")


def header_stricter():
    """The STRICTER lines of include/ndnet_ingest.h: ``{key: "PARSE" | "CLASS"}``."""
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ndnet_ingest.h")).read()
    return dict(re.findall(r"^ \*\s+STRICTER (\w+)\s+(PARSE|CLASS)\s", hdr, re.M))


def oracle(raw, header_lines, num_classes, errors="strict"):
    """``("ok", xyz, tags)`` or ``("raise", exception, index or None)`` of the oracle's parse."""
    try:
        xyz, tags = O.parse_bytes(raw, num_classes, header_lines, errors)
    except O.LineError as e:
        return "raise", e.__cause__, e.index
    except UnicodeDecodeError as e:  # the whole file fails to open as text
        return "raise", e, None
    return "ok", xyz, tags


def _case(name, raw, header_lines=HL, num_classes=NC, why=None, at=None):
    res = oracle(raw, header_lines, num_classes)
    if res[0] == "raise" and isinstance(res[1], UnicodeDecodeError):
        assert why is None, name
        return Case(name, bytes(raw), header_lines, num_classes, "not_utf8", None, None)
    if res[0] == "raise":
        # the one exception of the header: a non-ASCII line is not decoded, and is malformed even
        # where the reference, reading on, raises its class error
        assert why is None or (why in NOT_DECODED and not raw.isascii()), name
        kind = "both_fail"
    else:
        kind = "stricter" if why else "same"
    assert why is None or (why in STRICTER and (at is not None or kind == "both_fail")), name
    return Case(name, bytes(raw), header_lines, num_classes, kind, why, at)


def expected(case):
    """What the reader has to return: ``(0, xyz, tags)``, or ``(code, index)`` with ``index`` None
    where the oracle gives none (a file that does not decode)."""
    res = oracle(case.raw, case.header_lines, case.num_classes,
                 "surrogateescape" if case.kind == "not_utf8" else "strict")
    if case.kind == "same" or (case.kind == "not_utf8" and res[0] == "ok"):
        return OK, res[1], np.asarray(res[2], np.uint16)
    if case.kind == "stricter":  # the data lines the oracle counts ahead of the refused one
        before = oracle(case.raw[:case.at], case.header_lines, case.num_classes)
        return CODES[STRICTER[case.why]], len(before[2])
    exc, index = res[1], res[2]
    if case.why:
        return CODES[STRICTER[case.why]], index
    is_class = isinstance(exc, ValueError) and str(exc).startswith("Class tag")
    return (ERR_CLASS if is_class else ERR_PARSE), index


def same_bits(a, b):
    """float64 arrays equal bit for bit (the sign of zero included), NaN compared by position."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# ---------------------------------------------------------------------------------------------
# the reader at its C ABI, between sentinel pads

PAD = 64
XYZ_FILL = np.uint64(0x7FF8DEADBEEFCAFE)
CLS_FILL = np.uint16(0xA5C3)
Read = namedtuple("Read", "rc n xyz cls untouched")


def native_count(path, header_lines):
    from ndnet import _lib
    n = ctypes.c_uint64(0xDEAD)
    rc = _lib.lib().ndnet_ply_count(os.fsencode(str(path)), header_lines, ctypes.byref(n))
    return rc, n.value


def native_read(path, header_lines, num_classes, threads, capacity=None, extra=8):
    """``ndnet_ply_read`` into arrays of ``capacity`` rows (default: the count) that lie, with
    ``extra`` spare rows, between pads.  ``untouched`` says that the pads and, on success, every
    row from ``n`` on still hold the fill; on a failure, that nothing but rows below the count
    was written."""
    from ndnet import _lib
    lib = _lib.lib()
    bpath = os.fsencode(str(path))
    rc, count = native_count(path, header_lines)
    if rc:
        count = 0
    cap = count if capacity is None else capacity
    rows = max(cap, count) + extra
    xbuf = np.full(3 * (rows + 2 * PAD), XYZ_FILL, np.uint64)
    cbuf = np.full(rows + 2 * PAD, CLS_FILL, np.uint16)
    n = ctypes.c_uint64(0xDEAD)
    rc = lib.ndnet_ply_read(bpath, header_lines, num_classes, xbuf[3 * PAD:].ctypes.data, cbuf[PAD:].ctypes.data, cap,
                            ctypes.byref(n), threads)
    written = n.value if rc == OK else (0 if rc in (ERR_CAP, ERR_ARG, ERR_IO) else min(cap, count))
    lo = PAD + written
    untouched = bool((xbuf[:3 * PAD] == XYZ_FILL).all() and (xbuf[3 * lo:] == XYZ_FILL).all()
                     and (cbuf[:PAD] == CLS_FILL).all() and (cbuf[lo:] == CLS_FILL).all())
    got = n.value if rc == OK else 0
    xyz = xbuf[3 * PAD:3 * (PAD + got)].view(np.float64).reshape(-1, 3).copy()
    return Read(rc, n.value, xyz, cbuf[PAD:PAD + got].copy(), untouched)


# ---------------------------------------------------------------------------------------------
# number spellings

_R = np.random.default_rng(20240).standard_normal(6) * np.array([1e-3, 1.0, 80.0, 1e5, 1e17, 1e-17])
SPELLINGS = [
    # past and below double's range, and the edges of the range
    "1e999", "1e-999", "1e99999999999999999999", "1e-99999999999999999999", "0e999", "1" + "0" * 400,
    "0." + "0" * 400 + "1", "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "2e308",
    "2.2250738585072014e-308", "2.2250738585072011e-308", "2.2250738585072009e-308", "1e-310", "4.9e-324", "5e-324",
    "3e-324", "2.4703282292062328e-324", "2.4703282292062327e-324", "2e-324", "1e-400",
    # halfway cases of the correct rounding
    "9007199254740993", "9007199254740992.5", "9007199254740993.0000000000000000000000001", "9007199254740995",
    "1.00000000000000011102230246251565404236316680908203125",
    "1.000000000000000111022302462515654042363166809082031250000000000001",
    "1.00000000000000033306690738754696212708950042724609375", "0.1", "0.30000000000000004", "123456789012345678",
    # the words
    "inf", "Infinity", "INF", "iNfInItY", "nan", "NaN", "NAN", "infinit", "infinityx", "in", "na", "nane", "nan(1)",
    "nan()", "nan(abc)", "nan(", "inf(1)", "1inf", "infe5",
    # the shapes of a numeral
    "1.", ".5", ".5e1", "1e", "1e+", "1e-", "0x10", "0x1p3", "+1", "-1", "1e+05", "1E5", "1e5", "1.e5", ".e5", "e5",
    ".",
    "0", "0.0", "00012", "1..2", "1.2.3", "1e5.0", "1e5e5", "1e 5", "1,5", "1d5", "1f", "1L", "", "1_0", "1__0", "_1",
    "1_", "1_e5", "1e1_0", "1._5", "1_.5", "\u0661", "1\u0662", "\uff11",
] + [repr(float(v)) for v in _R]


def _twins(s):
    return [s, "+" + s, "-" + s]


@functools.lru_cache(maxsize=None)
def number_cases():
    """Each spelling and its signed twins as x, y or z of the second data line of a small file."""
    out = []
    for k, base in enumerate(SPELLINGS):
        for s in _twins(base):
            if not s:
                continue
            toks = ["1.5", "-2.25", "3"]
            toks[k % 3] = s
            first = "0.5 1 2 0.25 7 3\n"
            line = " ".join(toks) + " 0.5 9 4\n"
            raw = HEADER + (first + line + "6 7 8 9\n").encode("utf-8")
            why = None
            if oracle(raw, HL, NC)[0] == "ok":
                if "_" in s:
                    why = "underscore"
                elif not s.isascii():
                    why = "unicode_digit"
            out.append(_case(f"num[{s if len(s) < 40 else s[:20] + '..' + str(len(s))}]", raw, why=why,
                             at=len(HEADER) + len(first)))
    return out


# ---------------------------------------------------------------------------------------------
# class tags

TAGS = ["4", "+4", "-0", "+0", "0", "004", "4.0", "4.", "4e0", "0x4", "+-4", "-+4", "++4", "--4", "+", "-", "4-", "4+",
        "1_0", "1__0", "_4", "4_", "-1", "-28", "-1_0", "\u0664", "28", "29", "30", "65535", "65536",
        "9223372036854775807", "9223372036854775808", "18446744073709551616", "99999999999999999999",
        "+99999999999999999999", "-99999999999999999999", "-9223372036854775808", "-9223372036854775809", "inf", "nan"]


@functools.lru_cache(maxsize=None)
def tag_cases():
    out = []
    first = "0.5 1 2 0.25 7 3\n"
    at = len(HEADER) + len(first)
    for t in TAGS:
        raw = HEADER + (first + f"1 2 3 0.5 {t}\n5 6 7 8\n").encode("utf-8")
        why = None
        if oracle(raw, HL, NC)[0] == "ok":
            if "_" in t:
                why = "underscore"
            elif not t.isascii():
                why = "unicode_digit"
            elif t.startswith("-") and int(t) < 0:
                why = "negative_tag"
        out.append(_case(f"tag[{t}]", raw, why=why, at=at))
    # the bound: a tag equal to num_classes passes, one above it does not; 65535 is the largest
    for nc, t in ((5, 5), (5, 6), (0, 0), (0, 1), (65535, 65535), (65535, 65536), (65534, 65535), (-1, 0)):
        out.append(_case(f"tag_bound[{t},nc={nc}]", HEADER + f"1 2 3 {t}\n".encode(), num_classes=nc))
    return out


# ---------------------------------------------------------------------------------------------
# line structure

def _structure():
    H = HEADER
    good = b"1 2 3 4\n5.5 6.5 7.5 0.5 11 8\n"
    c = []
    add = lambda name, raw, **kw: c.append(_case("line[" + name + "]", raw, **kw))  # noqa: E731
    add("lone_cr", H.replace(b"\n", b"\r") + b"1 2 3 4\r5 6 7 8\r")
    add("lone_cr_no_final", H + b"1 2 3 4\r5 6 7 8")
    add("cr_then_lf_lines", H + b"1 2 3 4\r5 6 7 8\n9 10 11 12\r\n13 14 15 16\n\r17 18 19 20\r\r\n")
    add("crlf", H.replace(b"\n", b"\r\n") + good.replace(b"\n", b"\r\n"))
    add("crlf_header_lf_data", H.replace(b"\n", b"\r\n") + good)
    add("cr_header_crlf_data", H.replace(b"\n", b"\r") + good.replace(b"\n", b"\r\n"))
    add("no_final_newline", H + good[:-1])
    add("no_final_newline_cr", H + good[:-1] + b"\r")
    add("leading_trailing_blanks", H + b"  \t 1 2 3 4 \t \n\f\v5 6 7 8\v\f\n")
    add("tabs_and_form_feeds", H + b"1\t2\f3\v4\n5\t\t6 \f 7\v\v8\t\n")
    add("extra_columns", H + b"1 2 3 x y z !! 0.5 nan(1) 1_0 4\n1 2 3 4 5 6 7 8 9 10\n")
    add("four_tokens", H + b"1 2 3 4\n")
    add("blank_first", H + b"\n\n" + good)
    add("blank_last", H + good + b"\n\n\n")
    add("blank_middle", H + b"1 2 3 4\n\n \t \n\f\n5 6 7 8\n")
    add("blank_only", H + b"\n \n\t\n\r\n\v\f\n")
    add("cr_only_lines", H + b"1 2 3 4\n\r\n\r\r\n\r\n5 6 7 8\n\r")
    add("cr_only_file", b"\r\r\r\r\r\r", header_lines=2)
    add("empty_file", b"")
    add("empty_file_no_header", b"", header_lines=0)
    add("header_only", H)
    add("header_only_no_newline", H[:-1])
    add("header_longer_than_file", H + good, header_lines=50)
    add("header_zero", good, header_lines=0)
    add("header_zero_bad", H + good, header_lines=0)  # "ply" is no number
    add("header_one_short", H + good, header_lines=HL - 1)  # "end_header" is no number
    add("header_ten", b"h\n" * 10 + good, header_lines=10)
    # stricter than the reference: fewer than four tokens, other blanks, a NUL
    add("three_tokens", H + good + b"1 2 3\n", why="few_tokens", at=len(H + good))
    add("three_tokens_float_z", H + good + b"1 2 3.5\n")  # int("3.5") raises there too
    add("two_tokens", H + good + b"1 2\n")
    add("one_token", H + b"7\n")
    for ch in ("\x1c", "\x1d", "\x1e", "\x1f", "\x85", "\xa0", "\u1680", "\u2003", "\u3000"):
        b = ch.encode("utf-8")
        add(f"space_{ord(ch):04x}_before_tag", H + good + b"1 2 3" + b + b"4\n", why="other_space", at=len(H + good))
        add(f"space_{ord(ch):04x}_leading", H + good + b + b"1 2 3 4\n" + good, why="other_space", at=len(H + good))
        add(f"space_{ord(ch):04x}_in_x", H + b"1" + b + b"2 3 4 5\n", why="other_space", at=len(H))
        add(f"space_{ord(ch):04x}_only", H + good + b + b"\n" + good, why="other_space", at=len(H + good))
        add(f"space_{ord(ch):04x}_unread_column", H + b"1 2 3 0.5" + b + b"7 4\n")
    add("nul_unread_column", H + good + b"1 2 3 a\x00b 4\n", why="nul_byte", at=len(H + good))
    add("nul_alone_unread", H + b"1 2 3 \x00 4\n", why="nul_byte", at=len(H))
    add("nul_in_x", H + good + b"1\x00 2 3 4\n")
    add("nul_in_tag", H + good + b"1 2 3 4\x00\n")
    add("nul_only", H + good + b"\x00\n")
    add("nul_in_header", b"p\x00ly\nend\x00\nend_header\n" + good)
    add("not_utf8_in_z", H + good + b"1 2 \xff3 4\n")
    add("not_utf8_in_tag", H + good + b"1 2 3 4\xc3\n")
    add("not_utf8_unread_column", H + good + b"1 2 3 \xff 4\n" + good)
    add("not_utf8_in_header", b"ply\nformat \xff\xfe 1.0\nend_header\n" + good)
    add("not_utf8_unread_then_class", H + good + b"1 2 3 \xc3\x28 99\n")
    add("class_then_parse", H + good + b"1 2 3 99\n1 2 x 4\n")
    add("parse_then_class", H + good + b"1 2 x 4\n1 2 3 99\n")
    add("parse_and_class_one_line", H + good + b"1 2 x 99\n")
    # refused for the spelling, but the reference reads on and raises its class error: that one
    add("three_tokens_class", H + good + b"1 2 99\n")
    add("three_tokens_underscore_class", H + good + b"1 2 9_9\n")
    add("three_tokens_negative", H + good + b"1 2 -3\n", why="few_tokens", at=len(H + good))
    add("underscore_tag_class", H + good + b"1 2 3 0.5 9_9\n")
    add("underscore_tag_class_big", H + good + b"1 2 3 9_999_999_999_999_999_999_999\n")
    add("underscore_xyz_class", H + good + b"1_0 2_0.2_5 3e1_0 99\n")
    add("nul_unread_class", H + good + b"1 2 3 a\x00b 99\n")
    add("space_001c_class", H + good + b"1 2 3\x1c99\n")
    add("space_001f_three_tokens_class", H + good + b"1\x1f2\x1f99\n")
    add("non_ascii_unread_class", H + good + "1 2 3 \u00e9\u00a0\u0664 9_9\n".encode())
    add("space_00a0_class", H + good + "1 2 3\u00a099\n".encode(), why="other_space")
    add("unicode_digit_class", H + good + "1 2 3 \u0664\u0664\n".encode(), why="unicode_digit")
    add("stricter_parse_over_class", H + good + b"1 2 3 -1_0\n", why="underscore", at=len(H + good))
    return c


@functools.lru_cache(maxsize=None)
def structure_cases():
    return _structure()


# ---------------------------------------------------------------------------------------------
# the seeded grammar fuzz

FUZZ_LINES = 2000
FUZZ_SEED = 7
_ALPHABET = ["+", "-", ".", "e", "E", "_", "inf", "nan", "Infinity", "NaN"] + list("0123456789")
# digits carry most of the weight, so that about two thirds of the lines read; '_', the signs and
# the three-token lines are rare enough for the oracle alone to put well under a tenth of the
# lines on the stricter list
_WEIGHTS = [2, 2, 5, 3, 1, 0.4, 1, 1, 0.5, 0.5] + [4.5] * 10
_DIGITS = "0123456789"


def _numeral(rng):
    """A numeral of float()'s grammar, now and then with a '_' between two digits."""
    s = rng.choice(["", "", "", "-", "+"])
    s += "".join(rng.choices(_DIGITS, k=rng.randint(1, 8)))
    if len(s) > 2 and rng.random() < 0.008:
        s = s[:-1] + "_" + s[-1]
    if rng.random() < 0.6:
        s += "." + "".join(rng.choices(_DIGITS, k=rng.randint(0, 11)))
    if rng.random() < 0.3:
        s += rng.choice("eE") + rng.choice(["", "-", "+"]) + str(rng.randint(0, 399))
    return s


def _soup(rng):
    return "".join(rng.choices(_ALPHABET, _WEIGHTS, k=rng.randint(1, 5)))


def _fuzz_line(rng):
    ntok = rng.choices([3, 4, 5, 6], [0.05, 0.35, 0.2, 0.4])[0]
    toks = [(_soup(rng) if rng.random() < 0.08 else _numeral(rng)) for _ in range(ntok - 1)]
    r = rng.random()
    small = str(rng.randint(0, NC + 2))
    toks.append(small if r < 0.82 else _soup(rng) if r < 0.95 else rng.choice("+-") + small)
    sep = lambda: "".join(rng.choices(BLANKS, [0.7, 0.2, 0.05, 0.05], k=rng.randint(1, 2)))  # noqa: E731
    lead = sep() if rng.random() < 0.15 else ""
    trail = sep() if rng.random() < 0.15 else ""
    return lead + "".join(t + sep() for t in toks[:-1]) + toks[-1] + trail


def stricter_reason(line):
    """Why the reader refuses a fuzz line that the oracle reads, or None.  The alphabet has no
    other blank, no NUL and no non-ASCII digit, so three of the six reasons can occur; the PARSE
    reasons go first, as in the header."""
    toks = line.strip().split()
    if any("_" in t for t in toks[:3]):
        return "underscore"
    if len(toks) < 4:
        return "few_tokens"
    if "_" in toks[-1]:
        return "underscore"
    if int(toks[-1]) < 0:
        return "negative_tag"
    return None


Fuzz = namedtuple("Fuzz", "accepted refused n_same n_stricter n_both_fail")


@functools.lru_cache(maxsize=None)
def fuzz():
    """``accepted``: one ``same`` case holding every line that the oracle reads and the reader has
    to read.  ``refused``: one case per other line, a file of its own in which good lines and
    some blank lines stand before it, so that the reported index is not 0."""
    rng = random.Random(FUZZ_SEED)
    lines = [_fuzz_line(rng) for _ in range(FUZZ_LINES)]
    good, refused, n_stricter, n_both = [], [], 0, 0
    eols = ("\n", "\r\n", "\r")
    for k, ln in enumerate(lines):
        res = oracle(ln.encode(), 0, NC)
        why = stricter_reason(ln) if res[0] == "ok" else None
        if res[0] == "ok" and why is None:
            good.append(ln)
            continue
        n_stricter += res[0] == "ok"
        n_both += res[0] != "ok"
        eol = eols[k % 3]
        pad = ["1 2 3 4", "", "5 6 7 8", " \t", "9 10 11 12"][:k % 6]
        head = HEADER + "".join(p + eol for p in pad).encode()
        refused.append(_case(f"fuzz[{k}]", head + (ln + eol + "6 7 8 9" + eol).encode(), why=why, at=len(head)))
    accepted = _case("fuzz[accepted]", HEADER + "".join(g + "\n" for g in good).encode())
    assert accepted.kind == "same"
    return Fuzz(accepted, tuple(refused), len(good), n_stricter, n_both)


def all_cases():
    f = fuzz()
    return number_cases() + tag_cases() + structure_cases() + [f.accepted] + list(f.refused)


# ---------------------------------------------------------------------------------------------
# the structure of the parallel read: files whose cuts fall in chosen places.  The reader gives a
# thread at least CUT bytes and cuts the data at len * t / T, moved on to the next line start.

CUT = 65536
CR_LINE, CR_LINES = b"1.25 2.5 3.75 4\r", 1 << 18  # 16 bytes each: structure_files' cr_lines_4mb
EARLY, LATE = 300, 6 * CUT // 64 - 300  # the lines of structure_files' two errors


def _fixed_line(i, width=64):
    """Line i, ``width`` bytes with its newline, of full-precision numbers."""
    body = f"{i * 0.37 - 11.25!r} {-i * 1.5!r} {i % 97 + 0.125!r} {i % (NC + 1)}"
    return (body.ljust(width - 1) + "\n").encode()


@functools.lru_cache(maxsize=None)
def structure_files():
    """``{name: (raw, header_lines, num_classes)}``: every file reads, or fails, the same at
    every number of threads."""
    n6 = 6 * CUT // 64  # six ranges of 64 KB: the cuts of 2, 3 and 6 threads are line starts
    fixed = b"".join(_fixed_line(i) for i in range(n6))
    short = b"".join(f"{i} {i + 1} {i + 2} {i % 7}\n".encode() for i in range(2000))
    long_line = b"1.25" + b" " * 150_000 + b"2.5 3.75 " + b"0.5 " * 40_000 + b"\t 9\n"  # ~310 KB, one point
    blanks = b"\n \n\r\n\t\n" * (CUT // 8)  # 64 KB of nothing but blank lines
    files = {
        "fixed64": (fixed, 0, NC),  # no header, so the cuts are offsets into the file
        "fixed64_shifted": (b"\n" + fixed, 0, NC),
        "fixed64_header": (HEADER + fixed, HL, NC),
        "fixed64_crlf": (fixed.replace(b" \n", b"\r\n"), 0, NC),
        "fixed64_cr": (fixed.replace(b"\n", b"\r"), 0, NC),
        "long_line": (HEADER + short[:5000] + long_line + short, HL, NC),
        "long_line_last": (HEADER + short + long_line[:-1], HL, NC),
        "blank_runs": (HEADER + short + blanks + short + blanks + blanks + short[:700] + blanks, HL, NC),
        # 4 MB of short lines that end in a lone '\\r': read in time linear in the size
        "cr_lines_4mb": (HEADER + CR_LINE * CR_LINES, HL, NC),
        "just_under_64k": (fixed[:CUT - 64] + b"1 2 3 4" + b" " * 55 + b"\n", 0, NC),  # CUT - 1 bytes: one thread
        "exactly_64k": (fixed[:CUT], 0, NC),  # two threads
        "just_over_64k": (fixed[:CUT] + b"1 2 3 4\n", 0, NC),
    }
    assert len(files["just_under_64k"][0]) == CUT - 1 and len(fixed) >= 6 * CUT
    # two errors, in the first and in the last of six ranges, and each alone
    lines = [_fixed_line(i) for i in range(n6)]
    for name, e_line, l_line in (("class_early_parse_late", b"1 2 3 99", b"1 2 x 4"),
                                 ("parse_early_class_late", b"1 2 x 4", b"1 2 3 99"),
                                 ("class_late_only", None, b"1 2 3 99"), ("parse_late_only", None, b"1 2 x 4")):
        ls = list(lines)
        if e_line:
            ls[EARLY] = e_line.ljust(63) + b"\n"
        ls[LATE] = l_line.ljust(63) + b"\n"
        files[name] = (b"".join(ls), 0, NC)
    return files
