// ingest_main.cpp -- a stand-alone driver of the native PLY reader (include/ndnet_ingest.h) for
// tests/test_ingest_sanitized.py, which builds it together with ndt-net_amd/csrc/ply_ingest.cpp
// under AddressSanitizer + UBSan and under ThreadSanitizer.  Test code only: never linked into
// the library.
//
//   ingest_main PATH HEADER_LINES NUM_CLASSES THREADS [CAPACITY]
//   ingest_main @LIST      each line of LIST: HEADER_LINES NUM_CLASSES THREADS CAPACITY PATH
//
// For each call it runs ndnet_ply_count and ndnet_ply_read and prints one line
//   count_rc count read_rc n xyz_hash cls_hash
// CAPACITY -1 (the default) is the count.  The arrays hold exactly CAPACITY rows, so a write past
// them is the sanitizer's to report.  The hashes are of the rows [0, n) of a successful read
// (tests/test_ingest_sanitized.py computes the same of the plain library's arrays), else 0.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../include/ndnet_ingest.h"

namespace {

const uint64_t kMul = 0x9E3779B97F4A7C15ull;

// sum of (w ^ (w >> 31)) * (2 i + 1) * kMul over the words, modulo 2^64
uint64_t hash_add(uint64_t h, uint64_t i, uint64_t w) { return h + (w ^ (w >> 31)) * ((2 * i + 1) * kMul); }

int run(const std::string& path, int header_lines, int num_classes, int threads, long long capacity) {
  uint64_t count = 0;
  const int crc = ndnet_ply_count(path.c_str(), header_lines, &count);
  const uint64_t cap = capacity < 0 ? (crc == 0 ? count : 0) : (uint64_t)capacity;
  double* xyz = (double*)malloc(cap * 3 * sizeof(double));
  uint16_t* cls = (uint16_t*)malloc(cap * sizeof(uint16_t));
  if (!xyz || !cls) return 2;
  uint64_t n = 0;
  const int rc = ndnet_ply_read(path.c_str(), header_lines, num_classes, xyz, cls, cap, &n, threads);
  uint64_t hx = 0, hc = 0;
  if (rc == 0) {
    for (uint64_t i = 0; i < 3 * n; i++) {
      uint64_t w;
      memcpy(&w, &xyz[i], sizeof w);
      hx = hash_add(hx, i, w);
    }
    for (uint64_t i = 0; i < n; i++) hc = hash_add(hc, i, cls[i]);
  }
  printf("%d %" PRIu64 " %d %" PRIu64 " %016" PRIx64 " %016" PRIx64 "\n", crc, crc == 0 ? count : 0, rc, n, hx, hc);
  free(xyz);
  free(cls);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && argv[1][0] == '@') {
    std::ifstream list(argv[1] + 1);
    if (!list) return 2;
    std::string line;
    while (std::getline(list, line)) {
      if (line.empty()) continue;
      std::istringstream in(line);
      int header_lines, num_classes, threads;
      long long capacity;
      std::string path;
      if (!(in >> header_lines >> num_classes >> threads >> capacity)) return 2;
      in.get();  // the one blank before the path
      std::getline(in, path);
      if (int rc = run(path, header_lines, num_classes, threads, capacity)) return rc;
    }
    return 0;
  }
  if (argc < 5 || argc > 6) {
    fprintf(stderr, "usage: %s PATH HEADER_LINES NUM_CLASSES THREADS [CAPACITY] | @LIST\n", argv[0]);
    return 2;
  }
  return run(argv[1], atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argc == 6 ? atoll(argv[5]) : -1);
}
