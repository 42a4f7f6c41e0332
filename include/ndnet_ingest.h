/*
 * ndnet_ingest.h -- C ABI of the native ASCII-PLY reader in libndnet_amd.so
 * (ndt-net_amd/csrc/ply_ingest.cpp): the parsing half of the reference's
 * CARLA_Seg.get_data_pcl (ndnet/datasets/CARLA_Seg.py:97-136), which reads a
 * scan with Python readlines + split + float() per token.
 *
 * Semantics (same as the reference):
 *   - the first `num_header_lines` lines are skipped (default 10 there);
 *   - a line ends at "\n", at "\r\n" or at a lone "\r", as in Python's text
 *     mode (universal newlines): the header skip, the count, the range cuts
 *     and the parse all split at a lone "\r";
 *   - every further line gives x, y, z = its first three tokens, parsed as
 *     decimal -> double (correctly rounded, as Python float()) and the class
 *     tag = its LAST token, parsed as an integer (Python int());
 *   - float() spellings: an optional sign, then digits with an optional '.'
 *     and an optional exponent, or inf / infinity / nan in any letter case.
 *     A numeral past double's range gives +-inf, one below it +-0.0 or the
 *     correctly rounded subnormal, with the token's sign.  Anything else
 *     ("nan(1)", "+-1", "0x10", "1e") is a parse error;
 *   - int() spellings: an optional sign, then digits, of any length.  A tag
 *     too long for 64 bits is a class error like any tag > num_classes;
 *   - blank lines are skipped (the reference raises on them; a scan has none
 *     but possibly the last); a class tag > num_classes or a malformed number
 *     is an error, reported for the first such line in file order.
 *
 * Stricter than the reference -- the closed list of inputs that the
 * reference's loop reads and this reader refuses, each with the error code it
 * fails with (tests/ingest_cases.py holds the same list and
 * tests/test_ingest_cases.py compares the two):
 *   STRICTER few_tokens     PARSE  fewer than four tokens: the reference would read z as the tag
 *   STRICTER negative_tag   CLASS  a negative tag: it passes the reference's bound and fails its uint16 cast later
 *   STRICTER underscore     PARSE  '_' inside a numeral ("1_0"), which float() and int() drop
 *   STRICTER other_space    PARSE  whitespace other than space, \t, \r, \v, \f: bytes 0x1c-0x1f and the non-ASCII spaces
 *   STRICTER nul_byte       PARSE  a NUL byte anywhere in a data line (the reference ignores it in the unread columns)
 *   STRICTER unicode_digit  PARSE  non-ASCII decimal digits, which float() and int() take: the reader reads bytes, not code points, and no scan has them
 * Where a line is on the list for a PARSE and a CLASS reason ("1 2 3 -1_0"),
 * it fails with PARSE: a numeral is spelled right before its value is looked
 * at.  Where the reference reads a line of a PARSE entry as far as its class
 * bound and raises there ("1 2 99": z = tag = 99; "1 2 3 9_9"; a NUL in an
 * unread column in front of a tag 99), the reference does not read the line,
 * so it is not on the list, and the error is the reference's: CLASS.  The
 * reader finds that out by reading a line it has refused once more, the
 * reference's way.
 * The reader does not decode the file.  A line with a non-ASCII byte in a
 * token that is read is malformed (PARSE) even where the reference, splitting
 * at a non-ASCII space or reading non-ASCII digits, would get as far as its
 * class error: the first of two exceptions to the rule.
 * The second exception: bytes that are not UTF-8 fail the reference's open()
 * for the whole file, wherever they stand.  Here they fail only inside a
 * token that is read; in the header or in an unread column the file reads,
 * as the reference reads it when opened with errors="surrogateescape"
 * (tests/ingest_cases.py, kind not_utf8).
 * A limit of the interpreter, not of the reference's loop, is not followed:
 * where int() refuses a numeral of more than 4300 digits (Python's
 * int_max_str_digits), an all-digit tag of that length is still the class
 * error that its value makes it.
 *
 * The random subsample and the one-hot encoding (CARLA_Seg.py:137-175) stay
 * in Python (ndnet.datasets.carla_seg), on numpy's global RNG as there.
 * Parsing runs on `threads` host threads (0 or less = hardware concurrency,
 * at most one per 64 KB of data), each on a line-aligned byte range of the
 * memory-mapped file.
 */
#ifndef NDNET_INGEST_H_
#define NDNET_INGEST_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDNET_PLY_ERR_IO (-30)     /* open / map failure, or not a regular file */
#define NDNET_PLY_ERR_PARSE (-31)  /* malformed line; *n_out = its 0-based data-line index */
#define NDNET_PLY_ERR_CLASS (-32)  /* class tag > num_classes or < 0; *n_out = the data-line index */
#define NDNET_PLY_ERR_CAP (-33)    /* more data lines than `capacity`; *n_out = the count, nothing is written */

/* Counts the data lines (the non-blank lines after the header) of `path` into
 * *n_out.  -20 for a NULL argument or a negative num_header_lines. */
int ndnet_ply_count(const char *path, int num_header_lines, uint64_t *n_out);

/* Parses up to `capacity` data lines: xyz[i*3..] (double), cls[i] (uint16).
 * *n_out = the number of points on success; rows from there on are not
 * written.  -20 for a NULL argument, a negative num_header_lines or
 * num_classes > 65535 (a tag above that does not fit cls). */
int ndnet_ply_read(const char *path, int num_header_lines, int num_classes, double *xyz, uint16_t *cls,
                   uint64_t capacity, uint64_t *n_out, int threads);

#ifdef __cplusplus
}
#endif
#endif /* NDNET_INGEST_H_ */
