// Host harness for tests/test_cn_sign_magnitude.py: runs the check-node bodies of ldpc_dec_fast_core.h on random LDS images
// and prints one line per case with hashes of the message rows (wrap-around pad included) and of the returned flags.
// Compiled twice: as is (the bodies of the tree) and with -DCN_PARENT (ldpc_dec_fast_core_parent.h, a verbatim copy of the
// header before the sign-magnitude subtract); the test compares the two outputs line by line.
#ifdef CN_PARENT
#include "ldpc_dec_fast_core_parent.h"
#else
#include "ldpc_dec_fast_core.h"
#endif
#include <cstdio>
#include <cstring>
#include <vector>

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{ // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
// corners: 0 = every byte uniform; 1 = every byte from the saturation corners; 2 = half and half
static uint8_t rnd_byte(int corners)
{
  static const uint8_t c[6] = {0, 1, 127, 128, 129, 255};
  if (corners == 1 || (corners == 2 && (rnd() & 1)))
    return c[rnd() % 6];
  return (uint8_t)rnd();
}
static uint64_t fnv(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
  for (size_t i = 0; i < n; i++)
    h = (h ^ static_cast<const uint8_t *>(p)[i]) * 0x100000001b3ull;
  return h;
}

enum { Z = 32, RSTRIDE = Z + 4, NCORE = 19, MAXD = 19 };
// body: -1 = ldpc_fast_cn_dispatch, 0..2 = ldpc_fast_cn<.., MODE> called directly
template <bool P1>
static uint32_t run_item(int body, int deg, int ext, const ldpc_fast_lds &L, int j)
{
  if (body < 0)
    return ldpc_fast_cn_dispatch<P1>(deg, ext, L, 0, j, Z, RSTRIDE);
#define CN(D, E) \
  if (deg == D && ext == (E ? 1 : 0)) \
    return body == 0 ? ldpc_fast_cn<D, E, 0, P1>(L, 0, j, Z, RSTRIDE) : body == 1 ? ldpc_fast_cn<D, E, 1, P1>(L, 0, j, Z, RSTRIDE) \
                                                                                   : ldpc_fast_cn<D, E, 2, P1>(L, 0, j, Z, RSTRIDE);
  CN(3, true) CN(4, true) CN(6, true) CN(7, true) CN(8, false) CN(10, true) CN(19, false)
#undef CN
  return 0xdeadbeefu;
}

static int n_cases = 0;
static void run_case(int body, int deg, int ext, int p1, int ext_global, int corners)
{
  // LDS image: message rows | APP columns (stored twice) | extension LLRs | slack for the second dword of a window
  const int off_r = 0, off_app = off_r + MAXD * RSTRIDE, off_ext = off_app + NCORE * 2 * Z, total = off_ext + Z + 8;
  std::vector<uint32_t> mem32(total / 4 + 1), gl32(Z / 4 + 2);
  uint8_t *mem = reinterpret_cast<uint8_t *>(mem32.data()), *gl = reinterpret_cast<uint8_t *>(gl32.data());
  for (int i = 0; i < total; i++)
    mem[i] = rnd_byte(corners);
  for (int c = 0; c < NCORE; c++) // an APP column is stored twice back to back
    memcpy(mem + off_app + c * 2 * Z + Z, mem + off_app + c * 2 * Z, Z);
  for (int i = 0; i < Z + 8; i++)
    gl[i] = rnd_byte(corners);
  uint32_t etbl[MAXD];
  for (int k = 0; k < deg; k++)
    etbl[k] = (uint32_t)(off_app + k * 2 * Z) + rnd() % Z; // column k, some shift
  if (ext)
    etbl[deg - 1] = ext_global ? 4u : (uint32_t)off_ext;
  ldpc_fast_lds L;
  memset(&L, 0, sizeof(L));
  L.base = mem; L.r = mem + off_r; L.app = mem + off_app; L.ext = mem + off_ext;
  L.etbl = etbl; L.gllr = gl; L.ext_global = ext_global;
  uint32_t flags[Z / 4];
  for (int j = 0; j < Z / 4; j++)
    flags[j] = p1 ? run_item<true>(body, deg, ext, L, j) : run_item<false>(body, deg, ext, L, j);
  printf("body %d deg %d ext %d p1 %d extglobal %d corners %d : msgs %016llx flags %016llx\n", body, deg, ext, p1, ext_global, corners,
         (unsigned long long)fnv(mem + off_r, (size_t)deg * RSTRIDE), (unsigned long long)fnv(flags, sizeof(flags)));
  n_cases++;
}

int main()
{
#ifndef CN_PARENT
  { // (a) the sign-magnitude subtract against (0x8000 | a) - r -> (bit 15 clear = negative, |d|), all byte pairs, both halves
    unsigned bad = 0;
    auto ref = [](uint32_t a, uint32_t r) {
      const uint32_t d1 = ((0x8000u | a) - r) & 0xffffu;
      return (d1 & 0x8000u) ? d1 - 0x8000u : (0x8000u | (0x8000u - d1));
    };
    for (uint32_t a = 0; a < 256; a++)
      for (uint32_t r = 0; r < 256; r++) {
        const uint32_t a2 = (a * 7u + 3u) & 0xffu, r2 = 255u - r;
        bad += ldpc_psub_sm(a | (a2 << 16), r | (r2 << 16)) != (ref(a, r) | (ref(a2, r2) << 16));
        bad += ldpc_psub_sm(a2 | (a << 16), r2 | (r << 16)) != (ref(a2, r2) | (ref(a, r) << 16));
      }
    printf("psub_sm mismatches %u of 131072\n", bad);
  }
#endif
  for (int rep = 0; rep < 8; rep++)
    for (int corners = 0; corners < 3; corners++)
      for (int p1 = 0; p1 < 2; p1++) {
        // (b) every degree the dispatcher serves
        for (int deg = 3; deg <= 10; deg++)
          for (int eg = 0; eg < 2; eg++)
            run_case(-1, deg, 1, p1, eg, corners);
        for (int deg : {8, 10, 19})
          run_case(-1, deg, 0, p1, 0, corners);
        // the two-minima body in its three MODEs
        for (int mode = 0; mode < 3; mode++) {
          for (int deg : {3, 4, 6, 7, 10})
            for (int eg = 0; eg < 2; eg++)
              run_case(mode, deg, 1, p1, eg, corners);
          run_case(mode, 8, 0, p1, 0, corners);
          run_case(mode, 19, 0, p1, 0, corners);
        }
      }
  printf("cases %d\n", n_cases);
  return 0;
}
