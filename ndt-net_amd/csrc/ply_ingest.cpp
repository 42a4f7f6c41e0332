// ply_ingest.cpp -- native ASCII-PLY reader (include/ndnet_ingest.h), the
// parsing half of CARLA_Seg.get_data_pcl (ndnet/datasets/CARLA_Seg.py:97-136).
// The file is memory-mapped, the data lines are split into line-aligned
// byte ranges, and each range is parsed by its own thread into the output
// arrays at the range's first line index (a counting pass first).  A token is
// first checked against the spellings float() / int() take, then converted by
// std::from_chars (correctly rounded decimal -> double, like Python's float());
// the class tag is the line's last token as an integer (int()).
#include <charconv>
#include <cstdint>
#include <cstring>
#include <fcntl.h>
#include <locale.h>
#include <stdlib.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <utility>
#include <vector>

#include "../../include/ndnet_ingest.h"

namespace {

struct Mapped {
  const char* p = nullptr;
  size_t n = 0;
  int fd = -1;
  bool open(const char* path) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return false;
    n = (size_t)st.st_size;
    if (n == 0) return true;
    void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) return false;
    p = (const char*)m;
    return true;
  }
  ~Mapped() {
    if (p) munmap((void*)p, n);
    if (fd >= 0) close(fd);
  }
};

// One line of [a, b): *e = its end (the first '\n' or '\r', or b); returns the start of the next
// line.  A '\r' ends a line as a '\n' does (Python's universal newlines).  The '\n' of a "\r\n"
// pair then stands as an empty line of its own, which is blank and skipped like any other, so the
// count, the range cuts and the parse need no special case for the pair; only the header skip,
// which counts lines, does.
// The search goes block by block, so its cost is the line's length wherever the other kind of
// line end is (a file of "\r" lines has no '\n' at all).
inline const char* next_line(const char* a, const char* b, const char** e) {
  for (const char* c = a; c < b;) {
    const size_t k = (size_t)(b - c) < 4096 ? (size_t)(b - c) : 4096;
    const char* end = (const char*)memchr(c, '\n', k);
    const char* cr = (const char*)memchr(c, '\r', end ? (size_t)(end - c) : k);
    if (cr) end = cr;
    if (end) {
      *e = end;
      return end + 1;
    }
    c += k;
  }
  *e = b;
  return b;
}

// The lines of [a, b) one after the other, split as next_line splits them.  The next '\n' and the
// next '\r' are each looked for once and remembered until the walk has passed them, so every byte
// is searched at most twice, whatever the line ends are: a file with only one kind pays one
// search per range for the other, not one per line.
struct Lines {
  const char* a;
  const char* b;
  const char* nl = nullptr;  // the first '\n' at or after a (b: none); nullptr: not looked for yet
  const char* cr = nullptr;  // the same for '\r'
  bool any_cr = false;       // a search has found a '\r'
  Lines(const char* a_, const char* b_, bool no_cr = false) : a(a_), b(b_), cr(no_cr ? b_ : nullptr) {}
  // false at the end, else [*s, *e) is the next line
  bool next(const char** s, const char** e) {
    if (a >= b) return false;
    if (!nl || nl < a) {
      nl = (const char*)memchr(a, '\n', (size_t)(b - a));
      if (!nl) nl = b;
    }
    if (!cr || cr < a) {
      cr = (const char*)memchr(a, '\r', (size_t)(b - a));
      if (cr)
        any_cr = true;
      else
        cr = b;
    }
    const char* end = cr < nl ? cr : nl;
    *s = a;
    *e = end;
    a = end < b ? end + 1 : b;
    return true;
  }
};

// Offset just past the header's num_header_lines lines (the reference slices
// readlines()[num_header_lines:]); "\r\n" ends one line, not two.
size_t skip_header(const Mapped& m, int lines) {
  const char* a = m.p;
  const char* b = m.p + m.n;
  for (int i = 0; i < lines && a < b; i++) {
    const char* e;
    a = next_line(a, b, &e);
    if (e < b && *e == '\r' && a < b && *a == '\n') a++;
  }
  return (size_t)(a - m.p);
}

// The blanks between tokens.  Python's split() also takes 0x1c-0x1f and the non-ASCII spaces:
// those are refused here (ndnet_ingest.h, "stricter than the reference").  '\r' is on the header's
// list of blanks too, but ends a line before it can stand inside one.
inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f'; }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// A line is a data line unless it is all whitespace (Python's strip().split()
// of a blank line is empty and data[0] would raise; scans end with a newline,
// so the only blank line in practice is the final "").
inline bool blank(const char* a, const char* b) {
  for (; a < b; a++)
    if (!is_space(*a)) return false;
  return true;
}

// The data lines of [a, b); *no_cr = there is no '\r' in it (for the parse of the same range).
uint64_t count_lines(const char* a, const char* b, bool* no_cr) {
  uint64_t c = 0;
  Lines lines(a, b);
  const char* s;
  const char* e;
  while (lines.next(&s, &e))
    if (!blank(s, e)) c++;
  *no_cr = !lines.any_cr;
  return c;
}

inline bool word(const char* a, const char* e, const char* w) {  // case-insensitive, w in lower case
  for (; a < e && *w; a++, w++)
    if ((*a | 0x20) != *w) return false;
  return a == e && !*w;
}

// The spellings Python's float() takes of an ASCII token, minus '_' between digits (ndnet_ingest.h):
// [sign] (digits ['.' [digits]] | '.' digits) [('e'|'E') [sign] digits] | [sign] inf | infinity | nan.
// from_chars alone takes more ("nan(1)", "-1" after a skipped '+') and is not asked about those.
bool float_syntax(const char* a, const char* e) {
  if (a < e && (*a == '+' || *a == '-')) a++;
  if (word(a, e, "inf") || word(a, e, "infinity") || word(a, e, "nan")) return true;
  int nd = 0;
  for (; a < e && is_digit(*a); a++) nd++;
  if (a < e && *a == '.')
    for (a++; a < e && is_digit(*a); a++) nd++;
  if (!nd) return false;
  if (a < e && (*a | 0x20) == 'e') {
    a++;
    if (a < e && (*a == '+' || *a == '-')) a++;
    if (a == e) return false;
    for (; a < e && is_digit(*a); a++) {}
  }
  return a == e;
}

// A numeral outside double's range, where from_chars gives no value (libstdc++ also reports a
// result in the subnormal range so): strtod in the "C" locale rounds it correctly, to +-inf,
// a subnormal or +-0 with the token's sign, as float() does.
double out_of_range_double(const char* a, const char* e) {
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  const std::string s(a, e);
  return c_locale ? strtod_l(s.c_str(), nullptr, c_locale) : strtod(s.c_str(), nullptr);
}

// The token starting at a (not a blank) as float() reads it; returns its end, or nullptr.
// from_chars is asked first, and what it takes beyond float() is refused after it: a '-' after
// the '+' skipped for it ("+-1"), and "nan(...)", the one spelling of its that ends with ')'.
// The rest of float_syntax it checks itself: it stops where the numeral stops, and that has to
// be the token's end.
inline const char* parse_double(const char* a, const char* e, double& v) {
  const char* s = a;
  if (*s == '+' && ++s < e && *s == '-') return nullptr;  // from_chars does not take '+'
  auto r = std::from_chars(s, e, v);
  if (r.ec == std::errc()) return (r.ptr < e && !is_space(*r.ptr)) || r.ptr[-1] == ')' ? nullptr : r.ptr;
  if (r.ec != std::errc::result_out_of_range) return nullptr;
  const char* t = a;
  while (t < e && !is_space(*t)) t++;
  if (!float_syntax(a, t)) return nullptr;
  v = out_of_range_double(s, t);
  return t;
}

// The token [t0, t1) as int() reads it and the reference bounds it: [sign] digits, of any length.
// 0 ok, else an NDNET_PLY_ERR_* code.
inline int parse_tag(const char* t0, const char* t1, int num_classes, long long& tag) {
  if (t0 < t1 && *t0 == '+' && ++t0 < t1 && *t0 == '-') return NDNET_PLY_ERR_PARSE;  // from_chars takes no '+'
  auto r = std::from_chars(t0, t1, tag);
  if (r.ec == std::errc::result_out_of_range) {
    // all digits and past 64 bits: above any num_classes (CARLA_Seg.py:126-127), or below zero
    for (r.ptr = t0 + (*t0 == '-'); r.ptr < t1 && is_digit(*r.ptr);) r.ptr++;
    return r.ptr == t1 ? NDNET_PLY_ERR_CLASS : NDNET_PLY_ERR_PARSE;
  }
  if (r.ec != std::errc() || r.ptr != t1) return NDNET_PLY_ERR_PARSE;
  // CARLA_Seg.py:126-127; a negative tag fails the uint16 cast (:141)
  return tag > num_classes || tag < 0 ? NDNET_PLY_ERR_CLASS : 0;
}

// One data line [a, e): 0 and the point, else an NDNET_PLY_ERR_* code.
inline int parse_line(const char* a, const char* e, int num_classes, double* v, long long& tag) {
  const char* q = a;
  for (int k = 0; k < 3; k++) {
    while (q < e && is_space(*q)) q++;
    q = q < e ? parse_double(q, e, v[k]) : nullptr;
    if (!q) return NDNET_PLY_ERR_PARSE;
  }
  // the last token of the line
  const char* t1 = e;
  while (t1 > q && is_space(t1[-1])) t1--;
  const char* t0 = t1;
  while (t0 > q && !is_space(t0[-1])) t0--;
  if (t0 == t1) return NDNET_PLY_ERR_PARSE;  // fewer than four tokens: data[-1] would be z
  // a NUL anywhere in the line: in a token that is read it is no numeral, this is the rest
  if (memchr(q, 0, (size_t)(t0 - q))) return NDNET_PLY_ERR_PARSE;
  return parse_tag(t0, t1, num_classes, tag);
}

// [a, e) without the '_' that float() and int() drop: each between two digits.  False if one is not.
bool drop_underscores(const char* a, const char* e, std::string& out) {
  out.clear();
  for (const char* c = a; c < e; c++) {
    if (*c != '_')
      out.push_back(*c);
    else if (c == a || c + 1 == e || !is_digit(c[-1]) || !is_digit(c[1]))
      return false;
  }
  return true;
}

// Only for a line that parse_line refused as malformed: does the reference's loop read it as far
// as the class bound, and raise there?  Then the error is the reference's class error, although
// the line is refused for its spelling ("1 2 3 9_9", "1 2 99", "1 2 3 \0 99").  This reads the
// line as the reference does, for ASCII: split() also splits at 0x1c-0x1f, float() and int() drop
// '_' between digits, a NUL outside the tokens read is nothing, and data[-1] of three tokens is z.
// Nothing is decoded: a token with a non-ASCII byte stays malformed (ndnet_ingest.h).
bool reference_raises_class(const char* a, const char* e, int num_classes) {
  auto py_space = [](char c) { return is_space(c) || (c >= 0x1c && c <= 0x1f); };
  std::vector<std::pair<const char*, const char*>> tok;
  for (const char* c = a; c < e;) {
    if (py_space(*c)) {
      c++;
      continue;
    }
    const char* t = c;
    while (c < e && !py_space(*c)) c++;
    tok.emplace_back(t, c);
  }
  if (tok.size() < 3) return false;
  std::string s;
  for (int k = 0; k < 3; k++)
    if (!drop_underscores(tok[k].first, tok[k].second, s) || !float_syntax(s.data(), s.data() + s.size()))
      return false;
  if (!drop_underscores(tok.back().first, tok.back().second, s)) return false;
  long long tag = 0;
  return parse_tag(s.data(), s.data() + s.size(), num_classes, tag) == NDNET_PLY_ERR_CLASS && s[0] != '-';
}

// 0 ok, else an NDNET_PLY_ERR_* code; *bad = the failing line index.
int parse_range(const char* a, const char* b, bool no_cr, uint64_t line0, int num_classes, double* xyz,
                uint16_t* cls, uint64_t* bad) {
  uint64_t i = line0;
  Lines lines(a, b, no_cr);
  const char* e;
  while (lines.next(&a, &e)) {
    if (!blank(a, e)) {
      double v[3];
      long long tag = 0;
      if (int rc = parse_line(a, e, num_classes, v, tag)) {
        *bad = i;
        return rc == NDNET_PLY_ERR_PARSE && reference_raises_class(a, e, num_classes) ? NDNET_PLY_ERR_CLASS : rc;
      }
      xyz[3 * i + 0] = v[0];
      xyz[3 * i + 1] = v[1];
      xyz[3 * i + 2] = v[2];
      cls[i] = (uint16_t)tag;
      i++;
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int ndnet_ply_count(const char* path, int num_header_lines, uint64_t* n_out) {
  if (!path || !n_out || num_header_lines < 0) return -20;
  Mapped m;
  if (!m.open(path)) return NDNET_PLY_ERR_IO;
  const size_t o = skip_header(m, num_header_lines);
  bool no_cr;
  *n_out = count_lines(m.p + o, m.p + m.n, &no_cr);
  return 0;
}

int ndnet_ply_read(const char* path, int num_header_lines, int num_classes, double* xyz, uint16_t* cls,
                   uint64_t capacity, uint64_t* n_out, int threads) {
  if (!path || !xyz || !cls || !n_out || num_header_lines < 0) return -20;
  if (num_classes > 65535) return -20;  // cls is uint16: a tag above 65535 would wrap
  Mapped m;
  if (!m.open(path)) return NDNET_PLY_ERR_IO;
  const size_t o = skip_header(m, num_header_lines);
  const char* base = m.p + o;
  const size_t len = m.n - o;
  int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
  if (T < 1) T = 1;
  if ((size_t)T > len / 65536 + 1) T = (int)(len / 65536 + 1);  // >= 64 KB per thread
  // line-aligned ranges: each cut just past a '\n' or '\r'
  std::vector<const char*> cut(T + 1);
  cut[0] = base;
  cut[T] = base + len;
  for (int t = 1; t < T; t++) {
    const char* c = base + len * t / T;
    if (c < cut[t - 1]) c = cut[t - 1];
    const char* e;
    cut[t] = next_line(c, base + len, &e);
  }
  std::vector<uint64_t> cnt(T), first(T + 1, 0);
  std::vector<int> rc(T, 0);
  std::vector<char> no_cr(T, 0);  // the range holds no '\r' (not vector<bool>: one element per thread)
  std::vector<uint64_t> bad(T, 0);
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
      pool.emplace_back([&, t] {
        bool f;
        cnt[t] = count_lines(cut[t], cut[t + 1], &f);
        no_cr[t] = f;
      });
    for (auto& th : pool) th.join();
  }
  for (int t = 0; t < T; t++) first[t + 1] = first[t] + cnt[t];
  if (first[T] > capacity) {
    *n_out = first[T];
    return NDNET_PLY_ERR_CAP;
  }
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
      pool.emplace_back([&, t] {
        rc[t] = parse_range(cut[t], cut[t + 1], no_cr[t] != 0, first[t], num_classes, xyz, cls, &bad[t]);
      });
    for (auto& th : pool) th.join();
  }
  for (int t = 0; t < T; t++)
    if (rc[t]) {  // the first failing line in file order, as the reference's loop raises there
      *n_out = bad[t];
      return rc[t];
    }
  *n_out = first[T];
  return 0;
}

}  // extern "C"
