// Host harness for tests/test_dec_block_ends_emul.py: the homogeneous batch launch of the fast decoder (ldpc_decoder_fast.hip
// itself, with ldpc_dec_fast_block.h's prologue, warm-up request and hard decision as written) on the CPU through the host shim of
// tests/emul/hip_host, one real thread per work-item.  A stand-alone program, built plain and with -fsanitize=address,undefined and
// run directly, never loaded into Python.
//
//   dec_block_ends_harness BG Z R n_blocks numMaxIter warm_ahead llr_file
//
// llr_file: n_blocks rows of exactly num_llr int8.  They are decoded from a heap array of exactly that size, rows num_llr apart,
// so that a read behind the last row -- the warm-up request of a block past the end of the batch -- is a sanitizer report.  The
// output rows lie 8 bytes apart in an array prefilled with 0xAA that starts 4 bytes in front of row 0: every row has guard bytes
// on both sides, and with an odd number of output dwords every other row is 4-byte aligned and no more.  warm_ahead goes into
// the launch's arguments as the library's launcher would put it (ldpc_api.cpp launch_decoder: the workgroups resident at once); it
// is read by builds with -DLDPC_DEC_WARM=1, the arm in which a workgroup asks for the row of block blockIdx.x + warm_ahead.
// Prints "info num_llr out_bytes pitch threads ext_global", "iter <pass counts>", "out <the whole output array in hex>".
#include "dec_emul_common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "ldpc_decoder_fast.hip"

int main(int argc, char **argv)
{
  if (argc != 8) {
    fprintf(stderr, "usage: %s BG Z R n_blocks numMaxIter warm_ahead llr_file\n", argv[0]);
    return 2;
  }
  const int BG = atoi(argv[1]), Z = atoi(argv[2]), R = atoi(argv[3]), n = atoi(argv[4]), max_iter = atoi(argv[5]), warm = atoi(argv[6]);
  std::unique_ptr<ldpc_code_desc_t> d(new ldpc_code_desc_t);
  if (ldpc_build_code_desc_shape(BG, Z, R, LDPC_SHAPE_THROUGHPUT, d.get()) != 0 || !d->f_ok || n < 1) {
    fprintf(stderr, "no fast descriptor for BG %d Z %d R %d\n", BG, Z, R);
    return 2;
  }
  const size_t num_llr = (size_t)d->num_llr, ob = (num_llr + 31) / 32 * 4, pitch = ob + 8, total = 4 + (size_t)n * pitch;
  std::unique_ptr<int8_t[]> llr(new int8_t[(size_t)n * num_llr]), out(new int8_t[total]);
  std::unique_ptr<int32_t[]> it(new int32_t[n]);
  FILE *f = fopen(argv[7], "rb");
  if (!f || fread(llr.get(), 1, (size_t)n * num_llr, f) != (size_t)n * num_llr || fgetc(f) != EOF) {
    fprintf(stderr, "%s: not %d rows of %zu bytes\n", argv[7], n, num_llr);
    return 2;
  }
  fclose(f);
  memset(out.get(), 0xAA, total);
  for (int i = 0; i < n; i++)
    it[i] = -1;
  ldpc_dec_args a;
  memset(&a, 0, sizeof a);
  a.code = d.get();
  a.llr = llr.get();
  a.llr_stride = (uint32_t)num_llr;
  a.out = out.get() + 4;
  a.out_stride = (uint32_t)pitch;
  a.n_iter = it.get();
  a.num_max_iter = max_iter;
  a.warm_ahead = (uint32_t)warm;
  hip_host::launch_with_threads = true;
  if (ldpc_fast_kernel_init() != hipSuccess || ldpc_launch_dec_fast(a, *d, (uint32_t)n, nullptr) != hipSuccess) {
    fprintf(stderr, "launch failed\n");
    return 1;
  }
  printf("info %zu %zu %zu %d %d\niter", num_llr, ob, pitch, d->f_n_threads, d->f_ext_global);
  for (int i = 0; i < n; i++)
    printf(" %d", it[i]);
  printf("\nout ");
  for (size_t i = 0; i < total; i++)
    printf("%02x", (unsigned)(uint8_t)out[i]);
  printf("\n");
  return 0;
}
