/*
 * job_layout.h -- the layout of a call's job buffer: its arrays back to back in 16-byte granules, in the order the call adds
 * them; every add / zeros / reserve returns its part's offset, write() fills the staging area for the ONE upload of
 * upload_bytes().  Host only (no HIP): compiled and tested alone (tests/test_job_layout.py).  The vectors given to add() are
 * read by write(): they must live until then.
 */
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

class JobLayout {
public:
  static constexpr size_t GRANULE = 16;
  /* copied */
  template <class T> size_t add(const std::vector<T> &v) { return uploaded(v.data(), v.size() * sizeof(T)); }
  /* uploaded as zeros: the part's whole granules */
  size_t zeros(size_t bytes) { return uploaded(nullptr, bytes); }
  /* device only, not uploaded: state the kernels write before they read it.  Such parts come last (asserted: in front of an
   * uploaded part they would travel as whatever the staging area holds) */
  size_t reserve(size_t bytes) { return take(bytes); }
  size_t upload_bytes() const { return up_; }
  size_t device_bytes() const { return top_; }
  /* dst: upload_bytes() of staging memory.  The padding behind a copied part is not written */
  void write(uint8_t *dst) const
  {
    for (const Part &p : parts_)
      if (p.src)
        memcpy(dst + p.off, p.src, p.bytes);
      else
        memset(dst + p.off, 0, granules(p.bytes));
  }

private:
  struct Part { size_t off, bytes; const void *src; /* nullptr: zeros */ };
  std::vector<Part> parts_;
  size_t top_ = 0, up_ = 0;
  static size_t granules(size_t bytes) { return (bytes + GRANULE - 1) / GRANULE * GRANULE; }
  size_t take(size_t bytes)
  {
    const size_t o = top_;
    top_ += granules(bytes);
    return o;
  }
  size_t uploaded(const void *src, size_t bytes)
  {
    assert(up_ == top_); /* nothing reserved so far */
    const size_t o = take(bytes);
    up_ = top_;
    if (bytes)
      parts_.push_back(Part{o, bytes, src});
    return o;
  }
};
