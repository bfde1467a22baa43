// Host harness for tests/test_dec_edge_trim_emul.py: runs the bit-node and check-node bodies of ldpc_dec_fast_core.h on made-up
// LDS images and prints one line per case with hashes of what they wrote (APP rows resp. message rows, wrap-around copies
// included) and of the returned parity flags.  Compiled twice: as is (the bodies of the tree) and with -DEDGE_PARENT
// (ldpc_dec_fast_core_parent.h, a verbatim copy of the header before the per-edge instruction count was cut); the test compares
// the two outputs line by line.  The bit-node lines also carry the largest value the whole-word accumulator of the odd lanes
// (S1 + 2^8 S2 + 2^16 S3 over the column's edges and the LLR word) takes, computed here in 64 bits from the bytes themselves.
#ifdef EDGE_PARENT
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
static uint64_t fnv(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
  for (size_t i = 0; i < n; i++)
    h = (h ^ static_cast<const uint8_t *>(p)[i]) * 0x100000001b3ull;
  return h;
}

enum { Z = 32 };

// ---------------------------------------------------------------- bit nodes
// pattern of the message bytes: 0 = all 0xff, 1 = all 0x01, 2 = alternating 0xff / 0x00, 3 = alternating 0x00 / 0xff, 4 = random
static uint8_t msg_byte(int pat, int i)
{
  switch (pat) {
    case 0: return 0xff;
    case 1: return 0x01;
    case 2: return (i & 1) ? 0x00 : 0xff;
    case 3: return (i & 1) ? 0xff : 0x00;
    default: return (uint8_t)rnd();
  }
}
static int n_bn = 0;
static uint64_t at_max = 0;
// one column of degree `deg`, its list padded to `maxdeg` entries with the row of zero bytes; every edge's Z - shift has byte
// phase `phase` (4: mixed); nb blocks side by side in a row as in ldpc_dec_fast_mblock.h (nb = 1: the one-block kernels)
static void run_bn(int deg, int maxdeg, int phase, int pat, uint32_t llr_word, int nb)
{
  const int MAXDEG = 34, rstride = nb * (Z + 4), astride = nb * 2 * Z, col = 2, ncore = 4;
  const int off_r = 0, off_zero = off_r + MAXDEG * rstride, off_app = off_zero + rstride + 8, total = off_app + ncore * astride;
  std::vector<uint32_t> mem32(total / 4 + 4);
  uint8_t *mem = reinterpret_cast<uint8_t *>(mem32.data());
  for (int k = 0; k < deg; k++)
    for (int b = 0; b < nb; b++) {
      uint8_t *row = mem + off_r + k * rstride + b * (Z + 4);
      for (int i = 0; i < Z; i++)
        row[i] = msg_byte(pat, i);
      memcpy(row + Z, row, 4); // the wrap-around copy of lanes 0..3
    }
  memset(mem + off_app, 0x5a, (size_t)ncore * astride);
  uint32_t ctbl[2 * (3 + MAXDEG)];
  const int first = 3;
  int shift[MAXDEG];
  for (int k = 0; k < maxdeg; k++) {
    shift[k] = (int)(rnd() % Z);
    if (phase < 4)
      shift[k] = (shift[k] & ~3) | ((Z - phase) & 3); // (Z - shift) & 3 == phase
    const uint32_t x = (uint32_t)(Z - shift[k]);
    ctbl[2 * (first + k)] = x;
    ctbl[2 * (first + k) + 1] = (uint32_t)(k < deg ? off_r + k * rstride : off_zero) - (x & 3u);
  }
  ldpc_fast_lds L;
  memset(&L, 0, sizeof(L));
  L.base = mem; L.r = mem + off_r; L.app = mem + off_app; L.ctbl = ctbl;
  const uint32_t colrec = ((uint32_t)first << 16) | ((uint32_t)deg << 8) | (uint32_t)col;
  uint64_t worst = 0;
  for (int b = 0; b < nb; b++)
    for (int j = 0; j < Z / 4; j++) { // j = 0: the wrap item; j = Z / 4 - 1: the last one
      ldpc_fast_bn(L, colrec, maxdeg, j, Z, astride, llr_word, b * (Z + 4), b * 2 * Z);
      // the odd lanes' accumulator in 64 bits: bytes 1..3 of every window and of the biased LLR word
      uint64_t at = (llr_word ^ 0x80808080u) >> 8;
      for (int k = 0; k < deg; k++) {
        const uint8_t *row = mem + off_r + k * rstride + b * (Z + 4);
        uint32_t w = 0;
        for (int i = 0; i < 4; i++)
          w |= (uint32_t)row[(4 * j + i + Z - shift[k]) % Z] << (8 * i);
        at += w >> 8;
      }
      worst = at > worst ? at : worst;
    }
  at_max = worst > at_max ? worst : at_max;
  printf("bn deg %d maxdeg %d phase %d pat %d llr %08x nb %d : app %016llx at_max %llu wrapped %d\n", deg, maxdeg, phase, pat, llr_word, nb,
         (unsigned long long)fnv(mem + off_app, (size_t)ncore * astride), (unsigned long long)worst, worst >> 32 ? 1 : 0);
  n_bn++;
}

// ---------------------------------------------------------------- check nodes
enum { RSTRIDE = Z + 4, NCORE = 19, MAXD = 19 };
// corners: 0 = every byte uniform; 1 = every byte from the saturation corners; 2 = every byte 0x00 or 0xff
static uint8_t rnd_byte(int corners)
{
  static const uint8_t c[6] = {0, 1, 127, 128, 129, 255};
  if (corners == 1)
    return c[rnd() % 6];
  if (corners == 2)
    return (rnd() & 1) ? 0xff : 0x00;
  return (uint8_t)rnd();
}
// body: -2 = ldpc_fast_cn2_dispatch (two items per call), -1 = ldpc_fast_cn_dispatch, 0..2 = ldpc_fast_cn<.., MODE> directly
template <bool P1, bool SYN>
static void run_items(int body, int deg, int ext, const ldpc_fast_lds &L, uint32_t *flags)
{
  const int nj = Z / 4;
  if (body == -2) { // items j and j + nj / 2 together
    for (int j = 0; j < nj / 2; j++)
      flags[j] = ldpc_fast_cn2_dispatch<P1, SYN>(deg, L, 0, j, 0, j + nj / 2, Z, RSTRIDE, flags[j + nj / 2]);
    return;
  }
  for (int j = 0; j < nj; j++) {
    if (body < 0) {
      flags[j] = ldpc_fast_cn_dispatch<P1, SYN>(deg, ext, L, 0, j, Z, RSTRIDE);
      continue;
    }
    flags[j] = 0xdeadbeefu;
#define CN(D, E) \
  if (deg == D && ext == (E ? 1 : 0)) \
    flags[j] = body == 0   ? ldpc_fast_cn<D, E, 0, P1, SYN>(L, 0, j, Z, RSTRIDE) \
               : body == 1 ? ldpc_fast_cn<D, E, 1, P1, SYN>(L, 0, j, Z, RSTRIDE) \
                           : ldpc_fast_cn<D, E, 2, P1, SYN>(L, 0, j, Z, RSTRIDE);
    CN(3, true) CN(6, true) CN(10, true) CN(8, false) CN(19, false)
#undef CN
  }
}

static int n_cn = 0;
static void run_cn(int body, int deg, int ext, int p1, int syn, int ext_global, int corners)
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
  if (p1)
    syn ? run_items<true, true>(body, deg, ext, L, flags) : run_items<true, false>(body, deg, ext, L, flags);
  else
    syn ? run_items<false, true>(body, deg, ext, L, flags) : run_items<false, false>(body, deg, ext, L, flags);
  printf("cn body %d deg %d ext %d p1 %d syn %d extglobal %d corners %d : msgs %016llx flags %016llx\n", body, deg, ext, p1, syn, ext_global,
         corners, (unsigned long long)fnv(mem + off_r, (size_t)deg * RSTRIDE), (unsigned long long)fnv(flags, sizeof(flags)));
  n_cn++;
}

int main()
{
  // bit nodes: column degrees 1 .. 31, the list as long as the column and padded past the next multiple of four, every byte
  // phase of the shift and a mix, the message patterns, LLR bytes 0x7f and 0x80 (and a mixed word)
  for (int deg = 1; deg <= 31; deg++)
    for (int maxdeg : {deg, (deg + 4) / 4 * 4 + 1})
      for (int phase = 0; phase <= 4; phase++)
        for (int pat = 0; pat <= 4; pat++)
          for (uint32_t llr : {0x7f7f7f7fu, 0x80808080u, 0x807f807fu})
            run_bn(deg, maxdeg, phase, pat, llr, 1);
  // several blocks per workgroup: the same through boff_r / boff_a
  for (int deg : {1, 3, 4, 5, 9, 23, 30, 31})
    for (int pat : {0, 4})
      for (uint32_t llr : {0x7f7f7f7fu, 0x80808080u})
        run_bn(deg, deg + 2, 4, pat, llr, 3);
  printf("bn cases %d at_max %llu\n", n_bn, (unsigned long long)at_max);
  // check nodes: every degree of the dispatchers, first pass and later ones, with the parity and without
  for (int rep = 0; rep < 4; rep++)
    for (int corners = 0; corners < 3; corners++)
      for (int p1 = 0; p1 < 2; p1++)
        for (int syn = 0; syn < 2; syn++) {
          for (int deg = 3; deg <= 10; deg++)
            for (int eg = 0; eg < 2; eg++)
              run_cn(-1, deg, 1, p1, syn, eg, corners);
          for (int deg : {8, 10, 19})
            run_cn(-1, deg, 0, p1, syn, 0, corners);
          for (int deg = 3; deg <= 5; deg++)
            for (int eg = 0; eg < 2; eg++)
              run_cn(-2, deg, 1, p1, syn, eg, corners);
          // the two-minima body (the degree-19 rows of the general builds) in its three MODEs
          for (int mode = 0; mode < 3; mode++) {
            for (int deg : {3, 6, 10})
              for (int eg = 0; eg < 2; eg++)
                run_cn(mode, deg, 1, p1, syn, eg, corners);
            run_cn(mode, 8, 0, p1, syn, 0, corners);
            run_cn(mode, 19, 0, p1, syn, 0, corners);
          }
        }
  printf("cn cases %d\n", n_cn);
  return at_max >> 32 ? 1 : 0;
}
