/*
 * slot_call.inc.cpp -- what the slot-level entry points share (included into ldpc_api.cpp behind tb_api.inc.cpp, whose TbCtx it
 * uploads descriptor tables through, and ahead of the *_api.inc.cpp files that use it): the scope of a DEVICE mem call and of a
 * HOST mem call, the layout of a call's descriptor tables, and the small checks and derivations that more than one of them needs.
 * An entry point reads top to bottom: checks, plan, one of the two scopes, launch, scatter.
 */

namespace {

int check_mem(const char *who, int32_t mem)
{
  if (mem != NRLDPC_HIP_MEM_HOST && mem != NRLDPC_HIP_MEM_DEVICE)
    return set_error((std::string(who) + ": mem must be NRLDPC_HIP_MEM_HOST or NRLDPC_HIP_MEM_DEVICE").c_str());
  return 0;
}

/* DEVICE mem: the HIP ordinal of the GPU whose memory holds p (hipMalloc or managed), -1 for anything else */
int scr_device_ordinal(const void *p)
{
  hipPointerAttribute_t at;
  if (p && hipPointerGetAttributes(&at, p) == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged))
    return at.device;
  (void)hipGetLastError();
  return -1;
}

/* ---- two arrays back to back, each padded to 16 bytes: a call's descriptor tables (the workgroup table, then the job table) or
 * its jobs and their state (b == nullptr: nb zeroed elements) ---- */
template <typename A, typename B> struct Table2 {
  const A *a;
  size_t na;
  const B *b;
  size_t nb;
  static size_t bytes(size_t na, size_t nb) { return align_up(na * sizeof(A), 16) + align_up(nb * sizeof(B), 16); }
  size_t bytes() const { return bytes(na, nb); }
  void write(uint8_t *dst) const
  {
    memcpy(dst, a, na * sizeof(A));
    if (b)
      memcpy(dst + align_up(na * sizeof(A), 16), b, nb * sizeof(B));
    else
      memset(dst + align_up(na * sizeof(A), 16), 0, align_up(nb * sizeof(B), 16));
  }
  /* the two parts of a copy at base */
  const A *first(const uint8_t *base) const { return reinterpret_cast<const A *>(base); }
  B *second(uint8_t *base) const { return reinterpret_cast<B *>(base + align_up(na * sizeof(A), 16)); }
};
template <typename A, typename B> Table2<A, const B> table2(const std::vector<A> &a, const std::vector<B> &b)
{
  return Table2<A, const B>{a.data(), a.size(), b.data(), b.size()};
}

/* ---- DEVICE mem: the call works in place on the caller's arrays, on the GPU that holds them and on the caller's stream ---- */
struct DevArray {
  const void *p; /* nullptr: an optional array that was not given */
  unsigned align;
};
struct DeviceCall {
  int ord = -1;
  hipStream_t s = nullptr; /* the caller's stream */
  std::optional<UseDevice> use;
  /* every array in the memory of the GPU that holds the first one, at its alignment; then that GPU for the rest of the scope.
   * needs: how the call's refusal words it */
  template <size_t N> int open(const char *who, const DevArray (&arrays)[N], const char *needs, void *stream)
  {
    ord = scr_device_ordinal(arrays[0].p);
    bool ok = ord >= 0 && (reinterpret_cast<uintptr_t>(arrays[0].p) & (arrays[0].align - 1u)) == 0;
    for (size_t i = 1; ok && i < N; i++)
      ok = !arrays[i].p || (scr_device_ordinal(arrays[i].p) == ord && (reinterpret_cast<uintptr_t>(arrays[i].p) & (arrays[i].align - 1u)) == 0);
    if (!ok)
      return set_error((std::string(who) + ": DEVICE mem needs " + needs).c_str());
    Device *dv = device_for_ordinal(ord);
    if (!dv)
      return -1;
    use.emplace(*dv);
    s = static_cast<hipStream_t>(stream);
    return 0;
  }
  /* the calls that upload descriptor tables do so through the thread's page-locked area: graph capture of them is not supported */
  int refuse_capture(const char *who)
  {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return set_error((std::string(who) + ": the stream is being captured (graph capture of this call is not supported)").c_str());
    }
    return 0;
  }
  /* the tables to the device, on the stream and ahead of the launches: their device copy, nullptr + error when that fails */
  template <typename T> uint8_t *upload(const T &tables) { return upload(tables, tables.bytes()); }
  /* a call with more than two arrays lays them out with JobLayout (job_layout.h): still one upload */
  uint8_t *upload(const JobLayout &lay) { return upload(lay, lay.upload_bytes()); }
  template <typename T> uint8_t *upload(const T &tables, size_t bytes)
  {
    TbCtx &c = tls_tb;
    hipStream_t on;
    if (tb_begin(on, s, false) != 0 || tb_wait_upload(c) != 0 || c.jobs_h.ensure(bytes) != 0 || c.jobs_d.ensure(bytes) != 0)
      return nullptr;
    tables.write(c.jobs_h.p);
    return tb_upload_jobs(c, c.jobs_d.p, bytes, s) != 0 ? nullptr : c.jobs_d.p;
  }
};
const char *const DEV_NEEDS_IN_OUT = "`in` and `out` in device memory of one GPU";
const char *const DEV_NEEDS_ALIGNED = "every array in device memory of one GPU, 4-byte aligned";

/* ---- HOST mem: the call works on copies in the thread's staging buffers (ThreadCtx), on the primary device and the thread's own
 * stream, and returns when the result is back ---- */
struct StagedCall {
  std::optional<UseDevice> use;
  ThreadCtx *c = nullptr;
  size_t top = 0; /* of the input area */
  int open()
  {
    if (ensure_ready() != 0)
      return -1;
    use.emplace(g.dev[0]);
    c = &tls_ctx;
    return 0;
  }
  /* the next part of the input area: its offset, 16-byte aligned */
  size_t take(size_t bytes)
  {
    const size_t o = top;
    top += align_up(bytes, 16);
    return o;
  }
  /* the buffers for what was taken so far -- or for in_cap, where a call must have them before it can lay out its input -- and
   * for out_bytes of output.  The accessors hold from here on. */
  int ensure(size_t out_bytes, size_t in_cap = 0) { return c->ensure(std::max(top, in_cap), out_bytes); }
  uint8_t *h(size_t off) const { return c->h_in + off; }
  uint8_t *d(size_t off) const { return c->d_in + off; }
  uint8_t *h_out() const { return c->h_out; }
  uint8_t *d_out() const { return c->d_out; }
  hipStream_t stream() const { return c->stream; }
  /* the first in_bytes of the input area to the device, the launches, out_bytes back -- from the output area, or (in_place) from
   * the input area into its host side -- and the wait for them */
  template <typename Launch> int run(size_t in_bytes, Launch launch, size_t out_bytes, bool in_place = false)
  {
    HIP_TRY(hipMemcpyAsync(c->d_in, c->h_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    if (launch() != 0)
      return -1;
    HIP_TRY(hipMemcpyAsync(in_place ? c->h_in : c->h_out, in_place ? c->d_in : c->d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
};

/* ---- the write set of a call: [lo, hi) ranges that must not overlap ---- */
struct Range64 {
  uint64_t lo, hi;
};
/* true when two of the ranges overlap (r comes back sorted); lo, hi: the span of all of them, UINT64_MAX and 0 when there are none */
bool ranges_overlap(std::vector<Range64> &r, uint64_t &lo, uint64_t &hi)
{
  lo = UINT64_MAX;
  hi = 0;
  for (const Range64 &x : r) {
    lo = std::min(lo, x.lo);
    hi = std::max(hi, x.hi);
  }
  std::sort(r.begin(), r.end(), [](const Range64 &a, const Range64 &b) { return a.lo < b.lo; });
  for (size_t i = 1; i < r.size(); i++)
    if (r[i].lo < r[i - 1].hi)
      return true;
  return false;
}

/* ---- DMRS sequences ---- */
/* c_init of the DMRS of one OFDM symbol, PUSCH and PDSCH alike (nr_gold.c:87-88, 107-108) */
uint32_t dmrs_c_init(uint32_t slot, uint32_t symbol, uint32_t scrambling_id, uint32_t scid)
{
  return (uint32_t)(((1ull << 17) * (NR_RXG_SYMBOLS * slot + symbol + 1u) * (2ull * scrambling_id + 1u) + 2ull * scrambling_id + scid) & 0x7fffffffull);
}
/* the sequence from symbol k on, two bits a symbol (the low two: the DMRS value of k itself), out of Gold words w0, w0 + 1, ...;
 * gold holds one word beyond the one k's bits lie in */
uint64_t dmrs_bits(const std::vector<uint32_t> &gold, uint32_t w0, uint32_t k)
{
  const uint32_t w = (k >> 4) - w0;
  return ((uint64_t)gold[w] | ((uint64_t)gold[w + 1] << 32)) >> ((2u * k) & 31u);
}
/* the words that hold symbols k0 .. k0 + n - 1 (n >= 1) and one more, for dmrs_bits; false when they cannot be generated */
bool dmrs_gold_words(uint32_t c_init, uint32_t k0, uint32_t n, std::vector<uint32_t> &gold, uint32_t &w0)
{
  w0 = k0 >> 4;
  gold.resize(((k0 + n - 1u) >> 4) - w0 + 2u);
  return nr_hip_gold_words(c_init, w0, (uint32_t)gold.size(), gold.data()) == 0;
}

/* ---- the builders of descriptors from an allocation ---- */
int alloc_check_symbols(const char *who, uint32_t start_symbol, uint32_t nr_of_symbols)
{
  if (nr_of_symbols == 0 || start_symbol >= NR_RXG_SYMBOLS || nr_of_symbols > NR_RXG_SYMBOLS - start_symbol)
    return set_error((std::string(who) + ": the symbols must lie within the slot's 14").c_str());
  return 0;
}
int alloc_check_width(const char *who, uint32_t rb_size, uint32_t fft_size, uint32_t first_carrier_offset)
{
  if (rb_size == 0)
    return set_error((std::string(who) + ": rb_size is 0").c_str());
  if (fft_size == 0 || (uint64_t)rb_size * 12u > fft_size)
    return set_error((std::string(who) + ": the allocation is wider than fft_size").c_str());
  if (first_carrier_offset >= fft_size)
    return set_error((std::string(who) + ": first_carrier_offset must be below fft_size").c_str());
  return 0;
}
/* the tail of a builder: nothing is written when the descriptors do not fit */
template <typename T> int emit_segments(const std::vector<T> &segs, T *seg_out, uint32_t cap, uint32_t *n_seg_out, const char *too_many)
{
  if (segs.size() > cap)
    return set_error(too_many);
  if (!segs.empty())
    memcpy(seg_out, segs.data(), segs.size() * sizeof segs[0]);
  *n_seg_out = (uint32_t)segs.size();
  return 0;
}

} // namespace
