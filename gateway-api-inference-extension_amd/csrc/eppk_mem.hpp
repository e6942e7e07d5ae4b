// eppk_mem.hpp -- who owns the library's device and pinned memory, and the one rule by which it grows ("Memory").
// Host-only: no HIP header, so tests/cpp/test_mem.cpp drives it with a counting policy under the sanitizers.
//
// A policy `Mem` supplies   static int  alloc(void** p, size_t bytes);      0 = ok
//                           static void release(void* p);
//                           static int  alias(void** dev, void* host);      the address the device uses for `host` (pinned memory;
//                                                                           device memory is its own alias)
#pragma once

#include <cstddef>
#include <initializer_list>
#include <string>

#include "../../include/eppk.h"

namespace eppk {

struct Member;
template <class Drain> int grow(Drain&& drain, size_t need, std::initializer_list<Member> bufs, bool* fresh = nullptr, std::string* err = nullptr);

// One allocation, untyped: the pointer, what the device calls it, its capacity in the units of its size rule, and its policy's calls.
class RawBuf {
 public:
  RawBuf(const RawBuf&) = delete;
  RawBuf& operator=(const RawBuf&) = delete;
  size_t cap() const { return cap_; }
  void reset() {
    if (p_) release_(p_);
    p_ = dev_ = nullptr; cap_ = 0;
  }

 protected:
  RawBuf(int (*a)(void**, size_t), void (*r)(void*), int (*l)(void**, void*)) : alloc_(a), release_(r), alias_(l) {}
  ~RawBuf() { reset(); }
  void take_from(RawBuf& o) { reset(); p_ = o.p_; dev_ = o.dev_; cap_ = o.cap_; o.p_ = o.dev_ = nullptr; o.cap_ = 0; }
  void* p_ = nullptr;
  void* dev_ = nullptr;
  size_t cap_ = 0;

 private:
  template <class Drain> friend int grow(Drain&&, size_t, std::initializer_list<Member>, bool*, std::string*);
  int (*alloc_)(void**, size_t);
  void (*release_)(void*);
  int (*alias_)(void**, void*);
};

// Its move-only, typed owner.
template <class T, class Mem>
class Buf : public RawBuf {
 public:
  Buf() : RawBuf(&Mem::alloc, &Mem::release, &Mem::alias) {}
  Buf(Buf&& o) noexcept : Buf() { take_from(o); }
  Buf& operator=(Buf&& o) noexcept { if (this != &o) take_from(o); return *this; }
  operator T*() const { return (T*)p_; }                                 // (so `c->d_x` reads as the raw pointer did ...
  template <class U> explicit operator U*() const { return (U*)p_; }     //  ... and so do the casts at the launch sites)
  T* operator->() const { return (T*)p_; }
  T* get() const { return (T*)p_; }
  T* dev() const { return (T*)dev_; }
};

// One buffer of a group, as grow() sees it: `unit` bytes per unit of the group's size rule; `name` goes into the error message.
struct Member { RawBuf& buf; size_t unit; const char* name; };

// THE growth rule.  The members share one size rule (`need` units, unit bytes each; zero units count as one).  Nothing happens while
// every member holds that much.  Otherwise all of them are replaced together: drain() first -- once, and only if a member holds memory
// that queued work may still read (no work can read a buffer that never existed) -- then every release, then every allocation; the
// capacities are set when all of them have succeeded.  If one fails, the whole group is left empty (capacity 0) and the call returns
// EPPK_ERR_NOMEM with *err naming the buffer and its bytes: a retry starts clean.  *fresh says whether the memory is new (the caller
// initialises it behind that answer).  A make-once group is a call with a fixed `need`.
template <class Drain>
int grow(Drain&& drain, size_t need, std::initializer_list<Member> bufs, bool* fresh, std::string* err) {
  const size_t units = need ? need : 1u;
  bool enough = true, held = false;
  for (const Member& m : bufs) { enough = enough && m.buf.cap_ >= units; held = held || m.buf.p_ != nullptr; }
  if (fresh) *fresh = false;
  if (enough) return EPPK_OK;
  if (held) { const int rc = drain(); if (rc) return rc; }
  for (const Member& m : bufs) m.buf.reset();
  for (const Member& m : bufs) {
    RawBuf& b = m.buf;
    bool failed = b.alloc_(&b.p_, units * m.unit) != 0;
    if (!failed && b.alias_(&b.dev_, b.p_) != 0) { b.release_(b.p_); failed = true; }      // (a pinned block the device cannot address is no use)
    if (failed) {
      b.p_ = b.dev_ = nullptr;
      for (const Member& f : bufs) f.buf.reset();
      if (err) *err = std::string(m.name) + ": no memory for " + std::to_string(units * m.unit) + " bytes";
      return EPPK_ERR_NOMEM;
    }
  }
  for (const Member& m : bufs) m.buf.cap_ = units;
  if (fresh) *fresh = true;
  return EPPK_OK;
}

}  // namespace eppk
