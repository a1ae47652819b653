// tests/emul/dev_buf_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The grow-only device buffer (3dworld_amd/csrc/terra_stage.hpp: dev_buf_t) over a fake backend that counts alloc / free / sync, hands out real heap blocks (so
// the address sanitizer sees a block freed twice, leaked or written after its release) and can be told to throw on the next alloc.
// Built with -fsanitize=address,undefined and run as a child process by tests/test_host_staging_emul.py; exit status 0 = every check held.
#include "../../3dworld_amd/csrc/terra_stage.hpp"
#include <new>
#include <stdio.h>
#include <stdlib.h>

struct fake_backend_t {
	int allocs = 0, frees = 0, syncs = 0, syncs_at_last_free = -1;
	bool fail_next = false;
	void sync() {++syncs;}
	void *alloc(size_t bytes) {
		if (fail_next) {fail_next = false; throw std::bad_alloc();}
		++allocs;
		return malloc(bytes ? bytes : 1);
	}
	void free(void *p) {++frees; syncs_at_last_free = syncs; ::free(p);}
};

static int failures = 0;
#define CHECK(cond) do {if (!(cond)) {fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures;}} while (0)

int main() {
	fake_backend_t be;
	terra::dev_buf_t b;
	CHECK(b.p == nullptr && b.bytes == 0);
	CHECK(b.grow(be, 0) == nullptr && be.allocs == 0); // nothing asked for, nothing held: no allocation

	// the first growth: one allocation, nothing to free, no sync
	void *const p1 = b.grow(be, 100);
	CHECK(p1 != nullptr && b.p == p1 && b.bytes == 100);
	CHECK(be.allocs == 1 && be.frees == 0 && be.syncs == 0);
	memset(p1, 0xA5, 100);

	// want <= bytes allocates nothing and hands back the same block
	CHECK(b.grow(be, 100) == p1 && b.grow(be, 1) == p1 && b.grow(be, 0) == p1);
	CHECK(b.bytes == 100 && be.allocs == 1 && be.frees == 0 && be.syncs == 0);

	// growing past the size: exactly one free, after exactly one sync, then one allocation
	void *const p2 = b.grow(be, 101);
	CHECK(p2 != nullptr && b.p == p2 && b.bytes == 101);
	CHECK(be.allocs == 2 && be.frees == 1 && be.syncs == 1 && be.syncs_at_last_free == 1);
	memset(p2, 0x5A, 101);

	// an allocation that throws leaves the buffer empty: the old block went once, no stale pointer or size
	be.fail_next = true;
	bool thrown = false;
	try {(void)b.grow(be, 4096);} catch (std::bad_alloc const &) {thrown = true;}
	CHECK(thrown);
	CHECK(b.p == nullptr && b.bytes == 0);
	CHECK(be.allocs == 2 && be.frees == 2 && be.syncs == 2 && be.syncs_at_last_free == 2);

	// the next growth allocates afresh (even a small one: the size did not survive the pointer), with nothing to free
	void *const p3 = b.grow(be, 8);
	CHECK(p3 != nullptr && b.p == p3 && b.bytes == 8);
	CHECK(be.allocs == 3 && be.frees == 2 && be.syncs == 2);
	memset(p3, 0x33, 8);

	// a throwing first allocation of an empty buffer: still empty, nothing freed
	terra::dev_buf_t e;
	be.fail_next = true;
	thrown = false;
	try {(void)e.grow(be, 16);} catch (std::bad_alloc const &) {thrown = true;}
	CHECK(thrown && e.p == nullptr && e.bytes == 0 && be.frees == 2);
	e.drop(be);
	CHECK(be.frees == 2); // (an empty buffer drops nothing)

	// drop and a second drop free once; the buffer grows again afterwards
	b.drop(be);
	CHECK(b.p == nullptr && b.bytes == 0 && be.frees == 3);
	b.drop(be);
	CHECK(be.frees == 3 && be.allocs == 3);
	void *const p4 = b.grow(be, 4);
	CHECK(p4 != nullptr && b.bytes == 4 && be.allocs == 4 && be.frees == 3);
	memset(p4, 0x44, 4);
	b.drop(be);
	CHECK(be.frees == 4 && be.allocs == be.frees); // (and the leak check of the address sanitizer agrees)

	if (failures) {fprintf(stderr, "dev_buf_main: %d check(s) failed\n", failures); return 1;}
	printf("dev_buf_main: ok\n");
	return 0;
}
