// split_main -- the range-split rule of okv_encode_split (objectkv_amd/csrc/okv_split.hpp) on
// the CPU, for tests/test_split_rule_host.py (built with -fsanitize=address,undefined).
//
// Input file (little-endian u64 words): the case count, then per case
//   nb, split_bytes, split_rows, BlockSize[nb], first_row[nb + 1], n_starts, starts[n_starts]
// where starts is tests/split_model.py's answer: the first block of every segment, then nb.
// Each case is computed three ways from the header -- the serial walk of split::next, and the
// pointer-jumping rounds (split::jump, split::rounds) with the nodes of a round visited in
// ascending and in descending order, so marks land both before and after they are read --
// and every result must equal the model's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "okv_split.hpp"

namespace {

struct Pre {
  const std::vector<uint64_t>* v;
  uint64_t operator()(uint64_t k) const { return v->at(k); }
};

bool read_words(FILE* f, std::vector<uint64_t>& out, uint64_t n) {
  out.resize(n);
  return n == 0 || fread(out.data(), 8, n, f) == n;
}

std::vector<uint64_t> by_jumping(const std::vector<uint32_t>& j0, uint64_t nb, bool descending) {
  std::vector<uint32_t> jk = j0, jn(nb + 1), mark(nb + 1, 0);
  mark[0] = 1;
  const uint32_t rounds = okv::split::rounds(nb);
  for (uint32_t r = 0; r < rounds; ++r) {
    for (uint64_t x = 0; x <= nb; ++x) {
      const uint64_t i = descending ? nb - x : x;
      uint32_t t = 0;
      jn[i] = okv::split::jump(jk.data(), i, &t);
      if (mark[i]) mark.at(t) = 1;
    }
    jk.swap(jn);
  }
  std::vector<uint64_t> starts;
  for (uint64_t i = 0; i <= nb; ++i)
    if (mark[i]) starts.push_back(i);
  return starts;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t ncases = 0;
  if (fread(&ncases, 8, 1, f) != 1) return 2;
  uint64_t checked = 0;
  for (uint64_t c = 0; c < ncases; ++c) {
    uint64_t hdr[3];
    if (fread(hdr, 8, 3, f) != 3) return 2;
    const uint64_t nb = hdr[0], sb = hdr[1], sr = hdr[2];
    std::vector<uint64_t> bs, first, want;
    uint64_t nw = 0;
    if (!read_words(f, bs, nb) || !read_words(f, first, nb + 1) || fread(&nw, 8, 1, f) != 1 ||
        !read_words(f, want, nw))
      return 2;
    std::vector<uint64_t> bpre(nb + 1, 0);
    for (uint64_t k = 0; k < nb; ++k) bpre[k + 1] = bpre[k] + bs[k];
    const Pre B{&bpre}, R{&first};
    std::vector<uint32_t> j0(nb + 1);
    for (uint64_t i = 0; i < nb; ++i) {
      const uint64_t e = okv::split::next(i, nb, sb, sr, B, R);
      if (e <= i || e > nb) {
        printf("case %llu: next(%llu) = %llu\n", (unsigned long long)c, (unsigned long long)i,
               (unsigned long long)e);
        return 1;
      }
      j0[i] = uint32_t(e);
    }
    j0[nb] = uint32_t(nb);
    std::vector<uint64_t> serial;
    for (uint64_t i = 0; i < nb; i = j0[i]) serial.push_back(i);
    serial.push_back(nb);
    const std::vector<uint64_t> up = by_jumping(j0, nb, false), down = by_jumping(j0, nb, true);
    if (serial != want || up != want || down != want) {
      printf("case %llu (nb %llu, bytes %llu, rows %llu): serial %d, ascending %d, descending %d\n",
             (unsigned long long)c, (unsigned long long)nb, (unsigned long long)sb,
             (unsigned long long)sr, int(serial == want), int(up == want), int(down == want));
      return 1;
    }
    ++checked;
  }
  fclose(f);
  // the meta head and the arena's alignment unit
  if (okv::split::meta_head(3, 5, 0) != 2 + 3 + 2 + 5 + 1 + 1 + 1 + 8 ||
      okv::split::meta_head(3, 5, 32) != 2 + 3 + 2 + 5 + 1 + 8 + 32 + 1 + 1 + 8 ||
      okv::split::round16(0) != 0 || okv::split::round16(1) != 16 ||
      okv::split::round16(16) != 16 || okv::split::round16(17) != 32 ||
      okv::split::rounds(0) != 0 || okv::split::rounds(1) != 1 || okv::split::rounds(3) != 2 ||
      okv::split::rounds(4) != 3 || okv::split::rounds(1025) != 11) {
    printf("meta_head / round16 / rounds\n");
    return 1;
  }
  printf("%llu cases: all checks passed\n", (unsigned long long)checked);
  return 0;
}
