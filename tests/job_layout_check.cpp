/* Stand-alone check of csrc/job_layout.h (tests/test_job_layout.py compiles and runs it):   job_layout_check SEED ROUNDS
 * Seeded random layouts -- copied parts of 4 / 8 / 12 / 24 / 48-byte elements, zero parts, reserved parts at the end, empty
 * parts of every kind -- against the plain align_up chain the call sites used to write out by hand. */
#include <cstdio>
#include <cstdlib>
#include <list>
#include <random>

#include "job_layout.h"

template <size_t N> struct El { uint8_t b[N]; };
static_assert(sizeof(El<12>) == 12 && sizeof(El<24>) == 24 && sizeof(El<48>) == 48, "element sizes");

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Want { size_t off, bytes; int kind; /* 0 copied, 1 zeros, 2 reserved */ const uint8_t *src; };

template <size_t N> struct Pool {
  std::list<std::vector<El<N>>> kept; /* (a list: the vectors stay where they are until write()) */
  const std::vector<El<N>> &make(std::mt19937 &rng, size_t n)
  {
    kept.emplace_back(n);
    for (El<N> &e : kept.back())
      for (uint8_t &x : e.b)
        x = (uint8_t)(1 + rng() % 255); /* never 0: a part that was zeroed instead of copied shows */
    return kept.back();
  }
};

static int fail(unsigned seed, int round, size_t part, const char *what)
{
  fprintf(stderr, "job_layout_check: seed %u round %d part %zu: %s\n", seed, round, part, what);
  return 1;
}

int main(int argc, char **argv)
{
  const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 1u;
  const int rounds = argc > 2 ? atoi(argv[2]) : 200;
  std::mt19937 rng(seed);
  size_t n_kind[3] = {0, 0, 0}, n_empty[3] = {0, 0, 0}, n_size[5] = {0, 0, 0, 0, 0};
  for (int round = 0; round < rounds; round++) {
    Pool<4> p4; Pool<8> p8; Pool<12> p12; Pool<24> p24; Pool<48> p48;
    JobLayout lay;
    std::vector<Want> want;
    size_t top = 0, up = 0;
    const size_t n_up = 1 + rng() % 12, n_res = rng() % 3;
    for (size_t k = 0; k < n_up + n_res; k++) {
      const int kind = k >= n_up ? 2 : (rng() % 4 == 0 ? 1 : 0);
      const size_t n = rng() % 4 == 0 ? 0 : 1 + rng() % 40; /* elements, or bytes / 4 of a zero or reserved part */
      size_t got, bytes;
      const uint8_t *src = nullptr;
      if (kind == 0) {
        const int sz = (int)(rng() % 5);
        n_size[sz]++;
        switch (sz) {
        case 0: { const auto &v = p4.make(rng, n); got = lay.add(v); bytes = n * 4; src = (const uint8_t *)v.data(); break; }
        case 1: { const auto &v = p8.make(rng, n); got = lay.add(v); bytes = n * 8; src = (const uint8_t *)v.data(); break; }
        case 2: { const auto &v = p12.make(rng, n); got = lay.add(v); bytes = n * 12; src = (const uint8_t *)v.data(); break; }
        case 3: { const auto &v = p24.make(rng, n); got = lay.add(v); bytes = n * 24; src = (const uint8_t *)v.data(); break; }
        default: { const auto &v = p48.make(rng, n); got = lay.add(v); bytes = n * 48; src = (const uint8_t *)v.data(); break; }
        }
      } else {
        bytes = n * 4;
        got = kind == 1 ? lay.zeros(bytes) : lay.reserve(bytes);
      }
      n_kind[kind]++;
      n_empty[kind] += bytes == 0;
      if (got != top) /* o_x = o_prev + align_up(n * sizeof(T), 16) */
        return fail(seed, round, k, "offset differs from the align_up chain");
      want.push_back(Want{top, bytes, kind, src});
      top += align_up(bytes, 16);
      if (kind != 2)
        up = top;
    }
    if (lay.upload_bytes() != up || lay.device_bytes() != top)
      return fail(seed, round, want.size(), "upload_bytes / device_bytes");
    const size_t canary = 64;
    std::vector<uint8_t> dst(up + canary, 0xC7);
    lay.write(dst.data());
    for (size_t k = 0; k < want.size(); k++) {
      const Want &w = want[k];
      if (w.kind == 0 && w.bytes && memcmp(dst.data() + w.off, w.src, w.bytes) != 0)
        return fail(seed, round, k, "copied part differs");
      /* a zero part: zero over its granules, as the call sites zeroed o_x .. o_next (what lies behind them is checked as the
       * next part, or as the canary; no copied byte is 0) */
      if (w.kind == 1)
        for (size_t q = 0; q < align_up(w.bytes, 16); q++)
          if (dst[w.off + q] != 0)
            return fail(seed, round, k, "zero part does not read zero");
    }
    for (size_t q = up; q < up + canary; q++)
      if (dst[q] != 0xC7)
        return fail(seed, round, want.size(), "canary behind upload_bytes() overwritten");
  }
  printf("ok rounds=%d copied=%zu zeros=%zu reserved=%zu empty_copied=%zu empty_zeros=%zu empty_reserved=%zu sizes=%zu,%zu,%zu,%zu,%zu\n",
         rounds, n_kind[0], n_kind[1], n_kind[2], n_empty[0], n_empty[1], n_empty[2], n_size[0], n_size[1], n_size[2], n_size[3], n_size[4]);
  return 0;
}
