// terra_stage.hpp -- host-only plumbing of the driver and of the host-pointer entry points: how several arrays share one grow-only device scratch buffer.
//   dev_buf_t       the one grow-only device buffer: grow(backend, bytes), drop(backend)
//   stage_up        the one rounding: every carved array starts on a 256-byte boundary
//   stage_layout_t  a running offset: add(pointer, count) hands out the next array, `total` is what the buffer must hold, bind(base) sets the pointers
//   host_stage_t    the device copies of a host-pointer entry point's arrays: declare, begin() (upload), dev<T>(), end() (download)
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <stdexcept>
#include <string.h>

namespace terra {

// A device buffer that only grows.  grow() of no more than it holds hands back what it holds; otherwise the old allocation goes first (after a sync: kernels in flight may
// still use it) and the buffer is empty while the new one is made, so an allocation that throws leaves an empty buffer, not a stale pointer or size.
// BE: anything with sync(), alloc(bytes) and free(pointer).
struct dev_buf_t {
	void *p = nullptr; size_t bytes = 0;
	template<class BE> void *grow(BE &be, size_t want) {
		if (want <= bytes) return p;
		if (p) {be.sync(); drop(be);}
		p = be.alloc(want); bytes = want;
		return p;
	}
	template<class BE> void drop(BE &be) {if (p) {void *const q = p; p = nullptr; bytes = 0; be.free(q);}}
};

inline size_t stage_up(size_t bytes) {return (bytes + 255) & ~(size_t)255;}

// Two phases, because a grow-only buffer may move when it grows: the arrays are added first, then the buffer is sized with `total` and the pointers are set.
struct stage_layout_t {
	enum {MAX_BOUND = 16};
	size_t total = 0;
	size_t add_bytes(size_t bytes) {size_t const o = total; total += stage_up(bytes); return o;} // -> the array's offset
	template<class T> void add(T *&p, size_t count) { // `p` is set by bind()
		if (nbound == MAX_BOUND) throw std::logic_error("stage_layout_t: too many arrays");
		where[nbound] = &p; offs[nbound++] = add_bytes(count*sizeof(T));
	}
	void bind(void *base) {for (int i = 0; i < nbound; ++i) {void *const a = (uint8_t *)base + offs[i]; memcpy(where[i], &a, sizeof(a));}}
private:
	void *where[MAX_BOUND]; size_t offs[MAX_BOUND]; int nbound = 0;
};

// The same two phases: first every array is declared (the returned slot names it), then begin() sizes the buffer once and uploads.  The buffer is the engine's
// grow-only host-grid scratch or, with `own`, an allocation of the call's own that goes with the object.
// A slot that is not `present` takes no part: no upload, no download, dev() is null -- so a caller states the condition of an optional array once.
template<class ENGINE> struct host_stage_t {
	enum {MAX_SLOTS = 24};
	struct slot_t {void const *src; void *dst; size_t bytes, off; bool present;};
	ENGINE &eng;
	static constexpr bool OWN_ALLOC = true;
	bool const own;
	slot_t slots[MAX_SLOTS];
	int count = 0;
	stage_layout_t lay;
	uint8_t *d = nullptr;
	explicit host_stage_t(ENGINE &e, bool own_alloc = false) : eng(e), own(own_alloc) {}
	host_stage_t(host_stage_t const &) = delete;
	~host_stage_t() {if (own && d) {try {eng.be.free(d);} catch (...) {}}}

	// the general form: uploaded from `src` and downloaded to `dst` where they are not null (they may be different host arrays, or a slice of one)
	int add(void const *src, void *dst, size_t bytes, bool present = true) {
		if (count == MAX_SLOTS) throw std::logic_error("host_stage_t: too many arrays");
		slots[count] = slot_t{src, dst, bytes, present ? lay.add_bytes(bytes) : 0, present};
		return count++;
	}
	int in(void const *h, size_t bytes)      {return add(h, nullptr, bytes);}                // read by the pass
	int opt_in(void const *h, size_t bytes)  {return add(h, nullptr, bytes, h != nullptr);}  // read where the caller has one
	int out(void *h, size_t bytes)           {return add(nullptr, h, bytes);}                // always written by the pass, handed back where the caller wants it
	int opt_out(void *h, size_t bytes)       {return add(nullptr, h, bytes, h != nullptr);}  // written only where the caller wants it
	int inout(void *h, size_t bytes, bool present = true) {return add(h, h, bytes, present);}
	int temp(size_t bytes)                   {return add(nullptr, nullptr, bytes);}          // device-only

	void begin() {
		d = (uint8_t *)(own ? eng.be.alloc(lay.total) : (void *)eng.host_grid_scratch(lay.total));
		for (int i = 0; i < count; ++i) {slot_t const &s = slots[i]; if (s.present && s.src && s.bytes) {eng.be.h2d(d + s.off, s.src, s.bytes);}}
	}
	template<class T> T *dev(int slot) const {return slots[slot].present ? (T *)(d + slots[slot].off) : nullptr;}
	void end() {
		for (int i = 0; i < count; ++i) {slot_t const &s = slots[i]; if (s.present && s.dst && s.bytes) {eng.be.d2h(s.dst, d + s.off, s.bytes);}}
	}
	// [n][capacity] records of which tile t holds counts[t] (a count may exceed the capacity): the counts first, then of every tile only the records the counts name --
	// the rest of the caller's array stays as it was.  Both slots are declared temp(): end() does not touch them
	template<class T> void end_counted(int recs, int counts, T *h_recs, uint32_t *h_counts, uint32_t n, uint32_t capacity) {
		eng.be.d2h(h_counts, dev<uint32_t>(counts), (size_t)n*4);
		for (uint32_t t = 0; t < n; ++t) {
			uint32_t const m = std::min(h_counts[t], capacity);
			if (m) {eng.be.d2h(h_recs + (size_t)t*capacity, dev<T>(recs) + (size_t)t*capacity, (size_t)m*sizeof(T));}
		}
	}
};

} // namespace terra
