/*
 * slot_call.inc.cpp -- what the slot-level entry points share (included into ldpc_api.cpp behind tb_api.inc.cpp, whose TbCtx it
 * uploads descriptor tables through, and ahead of the *_api.inc.cpp files that use it): the scope of a DEVICE mem call and of a
 * HOST mem call, and the small derivations that more than one of them needs.  The layout of a call's descriptor tables, the
 * overlap check and the checks that need no HIP call are in slot_plan.h, which the CPU emulation of the kernels shares.
 * An entry point reads top to bottom: checks, plan, one of the two scopes, launch, scatter.
 */

namespace {

/* DEVICE mem: the HIP ordinal of the GPU whose memory holds p (hipMalloc or managed), -1 for anything else */
int scr_device_ordinal(const void *p)
{
  hipPointerAttribute_t at;
  if (p && hipPointerGetAttributes(&at, p) == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged))
    return at.device;
  (void)hipGetLastError();
  return -1;
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
  template <size_t N> int open(const char *who, const DevArray (&arrays)[N], const char *needs, void *stream) { return open(who, arrays, N, needs, stream); }
  /* ... for a call body that more than one entry point shares: the list is as long as its caller makes it */
  int open(const char *who, const DevArray *arrays, size_t N, const char *needs, void *stream)
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
