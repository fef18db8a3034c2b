// getrows_cpu_bench.cpp -- the CPU side of tools/getrows_bench.py: GetRow
// (segment_reader.go:362-404) on the host for a batch of keys, on T threads: the floor
// search of okv_index.hpp, the CPU restatement's ReadBlockWithStat of that block
// (oref_read_block from oracle/build/liboref.so, Go allocation semantics: a measurement
// baseline, dlopen'ed by this tool only) and the bytes.Equal loop.  No filter (the
// synthetic segment has none), member keys drawn uniformly.  No GPU is used.
//
// build: tools/build_getrows_cpu_bench.sh   run: tools/getrows_cpu_bench [keys] [threads...]
// prints one line per block size and thread count.
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../objectkv_amd/csrc/okv_index.hpp"
#include "okv_host.h"
#include "okv_sst.h"

namespace {

typedef struct {
  uint8_t* key;
  uint64_t key_len;
  uint8_t* val;
  uint64_t val_len;
} oref_kv;
typedef struct {
  oref_kv* rows;
  uint64_t n, cap;
} oref_rows;
typedef int (*read_block_fn)(const uint8_t*, uint64_t, const okv_block_desc*, int, oref_rows*);
typedef void (*rows_free_fn)(oref_rows*);

void key_of(uint64_t i, uint8_t* k) {  // OKV_SYNTH_FIXED: 8 zero bytes + big-endian index
  std::memset(k, 0, 8);
  for (int b = 0; b < 8; ++b) k[8 + b] = uint8_t(i >> (56 - 8 * b));
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t nkeys = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100000;
  std::vector<int> threads;
  for (int i = 2; i < argc; ++i) threads.push_back(std::atoi(argv[i]));
  if (threads.empty()) threads = {1, 16};
  void* oref = dlopen("oracle/build/liboref.so", RTLD_NOW);
  read_block_fn oref_read = oref ? (read_block_fn)dlsym(oref, "oref_read_block") : nullptr;
  rows_free_fn oref_free = oref ? (rows_free_fn)dlsym(oref, "oref_rows_free") : nullptr;
  if (!oref_read || !oref_free) {
    std::fprintf(stderr, "oracle/build/liboref.so not built (make -C oracle)\n");
    return 1;
  }
  const uint64_t rows = 100000;
  const uint64_t cfg[2][2] = {{3584, 4096}, {57344, 65536}};
  for (const auto& c : cfg) {
    okv_writer* w = okv_synth_segment(OKV_SYNTH_FIXED, 1, rows, 0, c[0], c[1]);
    uint64_t dlen = 0;
    const uint8_t* data = okv_writer_data(w, &dlen);
    const uint64_t nb = okv_writer_num_blocks(w);
    std::vector<okv_block_desc> descs(nb);
    std::vector<std::vector<uint8_t>> fks(nb);
    for (uint64_t i = 0; i < nb; ++i) {
      uint64_t h, fl;
      const uint8_t* fk;
      okv_writer_block(w, i, &descs[i], &h, &fk, &fl);
      fks[i].assign(fk, fk + fl);
    }
    const auto file_key = [&](size_t i, const uint8_t** p, size_t* n) {
      *p = fks[i].data();
      *n = fks[i].size();
    };
    const std::vector<uint64_t> tree = okv::index::tree_order(nb, file_key);
    const auto tree_key = [&](size_t t, const uint8_t** p, size_t* n) { file_key(tree[t], p, n); };
    std::vector<uint64_t> idx(nkeys);
    std::mt19937_64 rng(7);
    for (uint64_t& x : idx) x = rng() % rows;
    for (int T : threads) {
      std::atomic<uint64_t> found{0};
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<std::thread> pool;
      for (int t = 0; t < T; ++t)
        pool.emplace_back([&, t]() {
          uint64_t f = 0;
          uint8_t key[16];
          for (uint64_t i = uint64_t(t); i < nkeys; i += uint64_t(T)) {
            key_of(idx[i], key);
            const size_t up = okv::index::upper(tree.size(), tree_key, key, 16);
            if (up == 0) continue;
            oref_rows r{nullptr, 0, 0};
            if (oref_read(data, dlen, &descs[tree[up - 1]], 0, &r) == 0)
              for (uint64_t j = 0; j < r.n; ++j)
                if (r.rows[j].key_len == 16 && std::memcmp(r.rows[j].key, key, 16) == 0) {
                  ++f;
                  break;
                }
            oref_free(&r);
          }
          found += f;
        });
      for (std::thread& th : pool) th.join();
      const double us =
          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      std::printf("cpu GetRow BlockSize %llu keys=%llu threads=%d: %.0f us total, %.3f us/key, "
                  "keys/s=%.4g found=%llu\n",
                  (unsigned long long)c[1], (unsigned long long)nkeys, T, us, us / double(nkeys),
                  double(nkeys) / us * 1e6, (unsigned long long)found.load());
      std::fflush(stdout);
    }
    okv_writer_free(w);
  }
  return 0;
}
