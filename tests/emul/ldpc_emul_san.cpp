/*
 * ldpc_emul_san.cpp -- the decoder's and the encoders' per-thread code (ldpc_emul.cpp: the kernel bodies of ldpc_dec_core.h,
 * ldpc_dec_fast_core.h, ldpc_enc_core.h, ldpc_enc_packed_core.h and ldpc_enc_packed32.h on the CPU) under AddressSanitizer and
 * UndefinedBehaviorSanitizer, next to the oracle's C sources in the same program, so the oracle is sanitized too.  A stand-alone
 * program built by tests/test_ldpc_emul_san.py.  The input of a decode is a heap allocation of exactly num_llr bytes, its
 * output one of exactly the mode's extent (4 ceil(num_llr / 32) bytes packed, num_llr bytes one bit per byte); an encoder reads
 * exactly ceil(K / 8) bytes and writes exactly (ncols - 2) Zc.  Every lifting size, both base graphs, three rates each, the
 * generic kernel and both shapes of the fast one, the three output modes, the CRC stop; results against the oracle.  Then the
 * chain's phases on exact buffers too: UL de-matching, plain, scrambled
 * and from a symbol record (run_dematch: ldpc_emul.cpp, tb_rx_scr_emul.cpp, tb_rx_sym_emul.cpp), DL bit selection (run_tx_select)
 * the DL symbol store (run_tx_sym: tb_tx_sym_emul.cpp) and the packed scrambled store (run_tx_scr: tb_tx_scr_emul.cpp).
 * Exit status 0 and nothing on stderr: clean.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "ldpc_graph.h"
#include "nr_coding_host.h"
#include "nr_qam.h"
#include "../../oracle/oracle_nr_coding.h"

extern "C" {
int ldpc_emul_decode(int, int, int, int, int, int, int, int, const int8_t *, int8_t *);
int ldpc_emul_decode_fast(int, int, int, int, int, int, int, int, const int8_t *, int8_t *);
void ldpc_emul_set_fast_shape(int);
int ldpc_emul_encode(int, int, int, const uint8_t *, uint8_t *);
int ldpc_emul_encode_packed(int, int, int, const uint8_t *, uint8_t *);
int ldpc_emul_encode_packed32(int, int, int, const uint8_t *, uint8_t *, int);
int tb_emul_rx_dematch_cut(uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, int, int, const int16_t *,
                           int16_t *, int8_t *);
int tb_emul_first_tx_columns(uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, int, uint32_t);
int tb_emul_rx_dematch_scr(uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, int, uint32_t, uint32_t, uint32_t, int, int, uint32_t, uint32_t,
                           const int16_t *, int16_t *, int8_t *);
int tb_emul_rx_dematch_sym(uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, int, uint32_t, uint32_t, uint32_t, int, int, uint32_t, uint32_t,
                           const int16_t *, uint32_t, int16_t *, int8_t *);
int tb_emul_tx_sym(const uint8_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int, uint32_t *);
int tb_emul_tx_scr(uint32_t, const uint32_t *, uint32_t, uint32_t, const uint8_t *, uint32_t, int, const uint32_t *, uint32_t, uint32_t *, uint32_t *,
                   uint32_t, uint32_t *, uint32_t, uint32_t *);
int tb_emul_tx_select(uint32_t, int, uint32_t, uint32_t, uint32_t, int, int, uint32_t, uint32_t, uint32_t, int, const uint8_t *, uint8_t *);
}

static long n_calls = 0, n_bad = 0;
static uint32_t rnd()
{
  static uint64_t s = 0x2545f4914f6cdd1dull;
  s ^= s << 13;
  s ^= s >> 7;
  s ^= s << 17;
  return (uint32_t)(s >> 20);
}
static void differs(const char *what, int BG, int Z, int R, int mode)
{
  fprintf(stderr, "%s BG %d Z %d R %d mode %d: differs from the oracle\n", what, BG, Z, R, mode);
  n_bad++;
}

static int ncols_of(int BG, int R) { return BG == 1 ? (R == 13 ? 68 : R == 23 ? 35 : 27) : (R == 15 ? 52 : R == 13 ? 32 : 17); }

/* UL de-matching (tb_rx_core.h: the fused segment kernel's prologue), a workgroup's threads walked phase by phase.  f is exactly
 * E int16, the segment's soft-buffer row exactly N = (66 | 50) Zc int16, the decoder input exactly num_llr int8 (the graph cut
 * behind the last column a first transmission reaches; the whole rate mode on a combining round).  Against the oracle's
 * nr_deinterleaving_ldpc -> rule R0 -> nr_rate_matching_ldpc_rx -> the caller's pack.  Qm 2..8, rv 0..3, LBRM on and off, E
 * below, at and above Ncb (several laps), one segment and several, both base graphs. */
static void run_dematch()
{
  static const struct {
    int BG;
    uint32_t A, lbrm;
  } tbs[] = {{1, 30000, 0}, {1, 30000, 24000}, {1, 9608, 9000}, {2, 5000, 6000}, {2, 3000, 0}, {2, 640, 0}};
  for (const auto &t : tbs) {
    unsigned Cn = 0, K = 0, Z = 0, F = 0;
    const unsigned B = t.A + (t.A > 3824 ? 24 : 16);
    if (oracle_nr_segmentation(nullptr, nullptr, B, &Cn, &K, &Z, &F, (uint8_t)t.BG) <= 0) {
      n_bad++;
      continue;
    }
    const uint32_t N = (t.BG == 1 ? 66u : 50u) * Z, Ncb = !t.lbrm ? N : (N < 3u * t.lbrm / (2u * Cn) ? N : 3u * t.lbrm / (2u * Cn));
    const int ncore = t.BG == 1 ? 26 : 14;
    for (uint32_t Qm = 2; Qm <= 8; Qm += 2)
      for (int rv = 0; rv < 4; rv++)
        for (int size = 0; size < 5; size++) {
          static const double rate[4] = {0.25, 0.6, 0.92, 0.08}; /* 0.08: E > Ncb, several laps */
          uint32_t E = size < 4 ? (uint32_t)((K - F) / rate[size]) / Qm * Qm : Ncb / Qm * Qm; /* the last: at Ncb */
          if (E < Qm * 4u)
            E = Qm * 4u;
          int llrLen = 0;
          const int R = oracle_nr_get_R_ldpc_decoder(rv, (int)E, t.BG, (int)Z, &llrLen, 0), ncols = ncols_of(t.BG, R);
          const int reach = tb_emul_first_tx_columns(t.lbrm, t.BG, Z, Cn, F, K, rv, E);
          if (reach <= 0) {
            n_bad++;
            continue;
          }
          const int ncut = ncols < (reach > ncore + 1 ? reach : ncore + 1) ? ncols : (reach > ncore + 1 ? reach : ncore + 1);
          const uint32_t np_mode = (uint32_t)ncols * Z - 2u * Z;
          std::unique_ptr<int16_t[]> f(new int16_t[E]), e(new int16_t[E]);
          for (uint32_t i = 0; i < E; i++)
            f[i] = (int16_t)((int)(rnd() % 600u) - 300);
          oracle_nr_deinterleaving_ldpc(E, (uint8_t)Qm, e.get(), f.get());
          for (int clear = 1; clear >= 0; clear--) {
            const int nc = clear ? ncut : ncols; /* a retransmission is never cut */
            std::unique_ptr<int16_t[]> w(new int16_t[N]), w0(new int16_t[N]), d(new int16_t[68 * 384]);
            for (uint32_t i = 0; i < N; i++)
              d[i] = w[i] = w0[i] = (int16_t)((int)(rnd() % 4000u) - 2000);
            if (clear)
              for (uint32_t i = Ncb; i < np_mode && i < N; i++)
                d[i] = 0; /* R0 */
            if (oracle_nr_rate_matching_ldpc_rx(t.lbrm, (uint8_t)t.BG, (uint16_t)Z, d.get(), e.get(), (uint8_t)Cn, (uint8_t)rv, (uint8_t)clear, E, F,
                                                K - F - 2u * Z) != 0) {
              n_bad++;
              continue;
            }
            std::unique_ptr<int8_t[]> l_ref(new int8_t[(size_t)nc * Z]), l(new int8_t[(size_t)nc * Z]);
            oracle_nr_llr_prepack(d.get(), l_ref.get(), t.BG, (int)Z, (int)K, (int)F, nc);
            memset(l.get(), 0x11, (size_t)nc * Z);
            const int span = tb_emul_rx_dematch_cut(t.lbrm, t.BG, Z, Cn, F, K, rv, E, Qm, (uint32_t)nc * Z, np_mode, clear, 256, f.get(), w.get(), l.get());
            n_calls++;
            if (span <= 0 || memcmp(w.get(), d.get(), (size_t)N * 2u) != 0 || memcmp(l.get(), l_ref.get(), (size_t)nc * Z) != 0)
              differs("rx_dematch", t.BG, (int)Z, R, (int)(Qm * 1000u + (uint32_t)rv * 100u + (uint32_t)size * 10u + (uint32_t)clear));
            /* the same segment scrambled, at codeword bit bit_off (tb_rx_scr_emul.cpp: the unscrambling flag of tb_rx_core.h), where
             * the graph is the whole rate mode's */
            if (nc == ncols && size != 3) {
              const uint32_t bit_off = (uint32_t)rv * 37u * Qm, c_init = (rnd() & 0x7fffffffu) | 1u, nw = (bit_off + E + 31u) / 32u;
              std::vector<uint32_t> gold(nw);
              if (nr_hip_gold_words(c_init, 0, nw, gold.data()) != 0) {
                n_bad++;
                continue;
              }
              std::unique_ptr<int16_t[]> fs(new int16_t[E]), w2(new int16_t[N]);
              for (uint32_t i = 0; i < E; i++)
                fs[i] = ((gold[(bit_off + i) >> 5] >> ((bit_off + i) & 31u)) & 1u) ? (int16_t)-f[i] : f[i];
              memcpy(w2.get(), w0.get(), (size_t)N * 2u);
              memset(l.get(), 0x11, (size_t)nc * Z);
              const int sp = tb_emul_rx_dematch_scr(t.lbrm, t.BG, Z, Cn, F, K, rv, E, Qm, (uint32_t)nc * Z, clear, 256, c_init, bit_off, fs.get(), w2.get(),
                                                    l.get());
              n_calls++;
              if (sp <= 0 || memcmp(w2.get(), d.get(), (size_t)N * 2u) != 0 || memcmp(l.get(), l_ref.get(), (size_t)nc * Z) != 0)
                differs("rx_dematch_scr", t.BG, (int)Z, R, (int)(Qm * 1000u + (uint32_t)rv * 100u + (uint32_t)size * 10u + (uint32_t)clear));
              /* and from a symbol record (tb_rx_sym_emul.cpp: the demapper as the source of phase A): Qm / 2 planes of exactly
               * E / Qm c16 each, the segment's symbols the whole record; full-scale values on every other size */
              const uint32_t S = E / Qm, np = Qm / 2u;
              std::unique_ptr<uint32_t[]> rec(new uint32_t[(size_t)np * S]);
              std::unique_ptr<int16_t[]> fd(new int16_t[E]), ed(new int16_t[E]), d2(new int16_t[68 * 384]);
              for (size_t i = 0; i < (size_t)np * S; i++)
                rec[i] = (size & 1) ? rnd() : (((rnd() % 600u) - (i < S ? 300u : 0u)) & 0xffffu) | ((((rnd() % 600u) - (i < S ? 300u : 0u)) & 0xffffu) << 16);
              for (uint32_t r = 0; r < S; r++) {
                uint32_t x[4] = {0, 0, 0, 0};
                for (uint32_t k = 0; k < np; k++)
                  x[k] = rec[(size_t)k * S + r];
                nr_qam_demap(Qm, x);
                for (uint32_t k = 0; k < np; k++) {
                  fd[r * Qm + 2u * k] = (int16_t)(uint16_t)x[k];
                  fd[r * Qm + 2u * k + 1u] = (int16_t)(uint16_t)(x[k] >> 16);
                }
              }
              if (nr_hip_gold_words(c_init, 0, (E + 31u) / 32u, gold.data()) != 0) {
                n_bad++;
                continue;
              }
              for (uint32_t i = 0; i < E; i++)
                if ((gold[i >> 5] >> (i & 31u)) & 1u)
                  fd[i] = (int16_t)(uint16_t)(0u - (uint32_t)(uint16_t)fd[i]);
              oracle_nr_deinterleaving_ldpc(E, (uint8_t)Qm, ed.get(), fd.get());
              for (uint32_t i = 0; i < N; i++)
                d2[i] = w2[i] = w0[i];
              if (clear)
                for (uint32_t i = Ncb; i < np_mode && i < N; i++)
                  d2[i] = 0;
              if (oracle_nr_rate_matching_ldpc_rx(t.lbrm, (uint8_t)t.BG, (uint16_t)Z, d2.get(), ed.get(), (uint8_t)Cn, (uint8_t)rv, (uint8_t)clear, E, F,
                                                  K - F - 2u * Z) != 0) {
                n_bad++;
                continue;
              }
              oracle_nr_llr_prepack(d2.get(), l_ref.get(), t.BG, (int)Z, (int)K, (int)F, nc);
              memset(l.get(), 0x11, (size_t)nc * Z);
              const int sy = tb_emul_rx_dematch_sym(t.lbrm, t.BG, Z, Cn, F, K, rv, E, Qm, (uint32_t)nc * Z, clear, 256, c_init, 0,
                                                    reinterpret_cast<const int16_t *>(rec.get()), 2u * S, w2.get(), l.get());
              n_calls++;
              if (sy <= 0 || memcmp(w2.get(), d2.get(), (size_t)N * 2u) != 0 || memcmp(l.get(), l_ref.get(), (size_t)nc * Z) != 0)
                differs("rx_dematch_sym", t.BG, (int)Z, R, (int)(Qm * 1000u + (uint32_t)rv * 100u + (uint32_t)size * 10u + (uint32_t)clear));
            }
          }
        }
  }
}

/* DL bit selection and interleaving (tb_tx_core.h: the fused segment kernel's gather and byte store) over the code word the
 * emulated encoder phases leave in LDS.  seg is exactly ceil(K / 8) bytes, f exactly E bytes.  Against the oracle's
 * encode -> nr_rate_matching_ldpc -> nr_interleaving_ldpc. */
static void run_tx_select()
{
  static const int codes[][4] = {{1, 6, 22, 0},  {1, 6, 22, 8},  {1, 36, 22, 40}, {1, 32, 22, 24}, {1, 64, 22, 56},
                                 {2, 6, 10, 0},  {2, 6, 6, 46},  {2, 36, 8, 88},  {2, 32, 9, 48},  {2, 64, 6, 296}};
  for (const auto &c : codes) {
    const int BG = c[0], Z = c[1], Kb = c[2], F = c[3], K = (BG == 1 ? 22 : 10) * Z, N = (BG == 1 ? 66 : 50) * Z;
    std::unique_ptr<uint8_t[]> seg(new uint8_t[(K + 7) / 8]), d(new uint8_t[(size_t)(BG == 1 ? 68 : 52) * Z]);
    memset(seg.get(), 0, (size_t)(K + 7) / 8);
    for (int i = 0; i < K - F; i++)
      if (rnd() & 1u)
        seg[i >> 3] |= (uint8_t)(0x80 >> (i & 7));
    oracle_ldpc_encode(BG, Z, Kb, seg.get(), d.get());
    const int Foffset = K - F - 2 * Z;
    for (int i = 0; i < F; i++)
      d[Foffset + i] = ORACLE_NR_NULL;
    for (uint32_t lbrm : {0u, (uint32_t)(2 * (K + Z + 5) + 2) / 3u}) {
      const uint32_t Ncb = !lbrm ? (uint32_t)N : ((uint32_t)N < 3u * lbrm / 2u ? (uint32_t)N : 3u * lbrm / 2u), V = Ncb - (uint32_t)F;
      for (uint32_t Qm = 2; Qm <= 8; Qm += 2) {
        const uint32_t sizes[8] = {Qm, Qm * 31u, Qm * 32u, Qm * 33u, Qm * 65u, (uint32_t)(0.6 * V) / Qm * Qm, (Ncb + 3u * Qm) / Qm * Qm,
                                   (2u * V + 37u + Qm) / Qm * Qm};
        for (uint32_t E : sizes)
          for (int rv = 0; rv < 4; rv++) {
            std::unique_ptr<uint8_t[]> e(new uint8_t[E]), want(new uint8_t[E]), got(new uint8_t[E]);
            const int rc = oracle_nr_rate_matching_ldpc(lbrm, (uint8_t)BG, (uint16_t)Z, d.get(), e.get(), 1, (uint32_t)F, (uint32_t)Foffset, (uint8_t)rv, E);
            if (rc == 0)
              oracle_nr_interleaving_ldpc(E, (uint8_t)Qm, e.get(), want.get());
            const uint32_t chunk = (rv & 1) ? 64u : 32u;
            memset(got.get(), 0x77, E);
            const int n = tb_emul_tx_select(lbrm, BG, (uint32_t)Z, 1, (uint32_t)F, Kb, rv, E, Qm, chunk, chunk == 32u ? 5 : 64, seg.get(), got.get());
            n_calls++;
            if (rc != 0 ? n != -1 : (n != (int)((E / Qm + chunk - 1u) / chunk) || memcmp(got.get(), want.get(), E) != 0))
              differs("tx_select", BG, Z, (int)E, (int)(Qm * 10u) + rv);
          }
      }
    }
  }
}

/* The symbol store of the fused DL segment kernel (tb_tx_sym_emul.cpp: tb_tx_sym.h): a segment's E bits, one per byte and exactly
 * E bytes, scrambled, mapped and layer-mapped into a record of exactly G / Qm words; two segments, the second from an odd bit
 * offset; chunks of 32 and 2048 symbols. */
static void run_tx_sym()
{
  static const nr_qam_tables_t tab = nr_qam_make_tables();
  for (uint32_t Qm = 2; Qm <= 8; Qm += 2)
    for (uint32_t Nl = 1; Nl <= 4; Nl++)
      for (uint32_t units : {1u, 7u, 1000u}) {
        const uint32_t unit = Qm * Nl, G = units * unit, S = G / Qm, plane = S / Nl, c_init = (rnd() & 0x7fffffffu) | 1u, nw = (G + 31u) / 32u;
        const uint32_t E0 = units > 1 ? (units / 3u) * unit : G, chunk = units == 7u ? 32u : 2048u;
        std::vector<uint32_t> gold(nw);
        if (nr_hip_gold_words(c_init, 0, nw, gold.data()) != 0) {
          n_bad++;
          continue;
        }
        std::unique_ptr<uint8_t[]> f0(new uint8_t[E0]), f1(new uint8_t[G - E0 ? G - E0 : 1]);
        std::unique_ptr<uint32_t[]> rec(new uint32_t[S]);
        memset(rec.get(), 0x5a, (size_t)S * 4u);
        for (uint32_t i = 0; i < G; i++)
          (i < E0 ? f0[i] : f1[i - E0]) = (uint8_t)(rnd() & 1u);
        int rc = tb_emul_tx_sym(f0.get(), E0, Qm, Nl, plane, c_init, 0, chunk, 64, rec.get());
        if (rc == 0 && G > E0)
          rc = tb_emul_tx_sym(f1.get(), G - E0, Qm, Nl, plane, c_init, E0, chunk, 64, rec.get());
        n_calls++;
        bool ok = rc == 0;
        for (uint32_t k = 0; k < S && ok; k++) {
          uint32_t x = 0;
          for (uint32_t b = 0; b < Qm; b++) {
            const uint32_t i = k * Qm + b;
            x |= (((i < E0 ? f0[i] : f1[i - E0]) ^ (gold[i >> 5] >> (i & 31u))) & 1u) << b;
          }
          ok = rec[(size_t)(k % Nl) * plane + k / Nl] == tab.pt[nr_qam_table_off(Qm) + x];
        }
        if (!ok)
          differs("tx_sym", 0, (int)G, (int)Qm, (int)Nl);
      }
}

/* The packed scrambled store of the fused DL segment kernel (tb_tx_scr_emul.cpp: tb_tx_scr.h): a block of several segments whose
 * boundaries fall inside words, chunk by chunk in two orders; the bits exactly G bytes, the output exactly ceil(G / 32) words, the
 * ticket and part arrays exactly as long as the plan says. */
static void run_tx_scr()
{
  for (uint32_t Qm = 2; Qm <= 8; Qm += 2)
    for (uint32_t chunk : {32u, 64u})
      for (int order = 0; order < 2; order++) {
        const uint32_t Cn = 4, Es[4] = {Qm * 33u, Qm * 7u, Qm * 150u, Qm * 65u}, c_init = (rnd() & 0x7fffffffu) | 1u;
        uint32_t G = 0;
        std::vector<uint32_t> steps;
        for (uint32_t q = 0; q < Cn; q++) {
          const uint32_t r = order ? Cn - 1u - q : q;
          G += Es[q];
          steps.insert(steps.end(), (Es[r] / Qm + chunk - 1u) / chunk, r);
        }
        const uint32_t nw = (G + 31u) / 32u;
        std::vector<uint32_t> gold(nw);
        std::unique_ptr<uint8_t[]> f(new uint8_t[G]);
        for (uint32_t i = 0; i < G; i++)
          f[i] = (uint8_t)(rnd() & 1u);
        uint32_t plan[2] = {0, 0};
        std::unique_ptr<uint32_t[]> out(new uint32_t[nw]), step_arr(new uint32_t[steps.size()]);
        memcpy(step_arr.get(), steps.data(), steps.size() * 4u);
        memset(out.get(), 0x5a, (size_t)nw * 4u);
        /* the plan's sizes first (nothing runs when the arrays are too short), then arrays of exactly those sizes */
        (void)tb_emul_tx_scr(Cn, Es, Qm, c_init, f.get(), chunk, 64, step_arr.get(), (uint32_t)steps.size(), out.get(), nullptr, 0, nullptr, 0, plan);
        std::unique_ptr<uint32_t[]> tickets(new uint32_t[plan[0] ? plan[0] : 1]), parts(new uint32_t[plan[1] ? plan[1] : 1]);
        memset(tickets.get(), 0, (size_t)(plan[0] ? plan[0] : 1) * 4u);
        memset(parts.get(), 0x5a, (size_t)(plan[1] ? plan[1] : 1) * 4u);
        const int rc = tb_emul_tx_scr(Cn, Es, Qm, c_init, f.get(), chunk, 64, step_arr.get(), (uint32_t)steps.size(), out.get(), tickets.get(), plan[0],
                                      parts.get(), plan[1], plan);
        n_calls++;
        bool ok = rc == 0 && plan[0] > 0 && nr_hip_gold_words(c_init, 0, nw, gold.data()) == 0;
        for (uint32_t i = 0; i < 32u * nw && ok; i++)
          ok = ((out[i >> 5] >> (i & 31u)) & 1u) == (i < G ? (uint32_t)(f[i] & 1u) ^ ((gold[i >> 5] >> (i & 31u)) & 1u) : 0u);
        for (uint32_t k = 0; k < plan[0] && ok; k++)
          ok = tickets[k] == 0; /* every ticket zero again for the next call */
        if (!ok)
          differs("tx_scr", rc, (int)G, (int)Qm, (int)chunk + order);
      }
}

int main()
{
  static const int sets[8] = {2, 3, 5, 7, 9, 11, 13, 15};
  static const int rates[2][3] = {{13, 23, 89}, {15, 13, 23}};
  for (int BG = 1; BG <= 2; BG++)
    for (int a = 0; a < 8; a++)
      for (int j = 0; j < 8; j++) {
        const int Z = sets[a] << j;
        if (Z > 384)
          continue;
        for (int ri = 0; ri < 3; ri++) {
          const int R = rates[BG - 1][ri];
          ldpc_code_desc_t d;
          if (ldpc_build_code_desc(BG, Z, R, &d) != 0) {
            n_bad++;
            continue;
          }
          const int num_llr = d.num_llr, E = (BG == 1 ? 22 : 10) * Z;
          /* a code word of zeros behind mild noise: it converges in a few passes, so the stop rules are reached; the first
           * decode of a code runs on noise alone, so every pass runs */
          std::unique_ptr<int8_t[]> llr(new int8_t[num_llr]);
          for (int kind = 0; kind < 2; kind++) {
            if (kind == 1 && (Z % 3 == 0 || ri != 0))
              continue; /* the second LLR kind on a third of the codes */
            for (int i = 0; i < num_llr; i++)
              llr[i] = kind ? (int8_t)rnd() : (int8_t)(12 + (int)(rnd() % 40u) - ((rnd() % 9u) == 0 ? 30 : 0));
            for (int mode = 0; mode < 3; mode++) /* packed bits; one bit per byte; LLRINT8, which the reference turns into bits too */
              for (int use_crc = 0; use_crc < 2; use_crc++) {
                if (use_crc && (kind || mode || E % 8 || E < 64))
                  continue; /* the CRC stop reads E / 8 whole bytes of the packed output, a 24-bit CRC among them */
                const size_t nb = mode == 0 ? 4u * (size_t)((num_llr + 31) / 32) : (size_t)num_llr;
                std::unique_ptr<int8_t[]> want(new int8_t[nb]), got(new int8_t[nb]);
                memset(want.get(), 0x5a, nb);
                const int it = oracle_ldpc_decode(BG, Z, R, 4, mode, use_crc, E, 1, llr.get(), want.get());
                for (int v = 0; v < 3; v++) {
                  if (v > 0 && (Z % 4 || Z < 8))
                    continue; /* the fast kernel's lifting sizes */
                  memset(got.get(), 0x5a, nb);
                  int rc;
                  if (v == 0)
                    rc = ldpc_emul_decode(BG, Z, R, 4, mode, use_crc, E, 1, llr.get(), got.get());
                  else {
                    ldpc_emul_set_fast_shape(v - 1);
                    rc = ldpc_emul_decode_fast(BG, Z, R, 4, mode, use_crc, E, 1, llr.get(), got.get());
                    if (rc == -2)
                      continue; /* no fast kernel for this code */
                  }
                  n_calls++;
                  if (rc != it || memcmp(got.get(), want.get(), nb) != 0)
                    differs(v == 0 ? "decode" : "decode_fast", BG, Z, R, mode + 10 * use_crc + 100 * v);
                }
              }
          }
        }
        /* the three encoders: ceil(K / 8) bytes in, (ncols - 2) Zc bytes out */
        const int Kb = BG == 1 ? 22 : 10, K = Kb * Z, n_out = ((BG == 1 ? 68 : 52) - 2) * Z;
        std::unique_ptr<uint8_t[]> in(new uint8_t[(K + 7) / 8]), want(new uint8_t[n_out]), got(new uint8_t[n_out]);
        for (int i = 0; i < (K + 7) / 8; i++)
          in[i] = (uint8_t)rnd();
        oracle_ldpc_encode(BG, Z, Kb, in.get(), want.get());
        for (int v = 0; v < 3; v++) {
          if (v == 2 && Z % 32)
            continue; /* the word-aligned encoder's lifting sizes */
          memset(got.get(), 0x5a, n_out);
          const int rc = v == 0   ? ldpc_emul_encode(BG, Z, Kb, in.get(), got.get())
                         : v == 1 ? ldpc_emul_encode_packed(BG, Z, Kb, in.get(), got.get())
                                  : ldpc_emul_encode_packed32(BG, Z, Kb, in.get(), got.get(), 0);
          n_calls++;
          if (rc != n_out || memcmp(got.get(), want.get(), n_out) != 0)
            differs(v == 0 ? "encode" : v == 1 ? "encode_packed" : "encode_packed32", BG, Z, 0, v);
        }
      }
  run_dematch();
  run_tx_select();
  run_tx_sym();
  run_tx_scr();
  printf("%ld calls, %ld mismatches\n", n_calls, n_bad);
  return n_bad == 0 && n_calls > 0 ? 0 : 1;
}
