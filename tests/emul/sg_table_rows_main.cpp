// tests/emul/sg_table_rows_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The bound on the sine-table rows that k_sine_grid's staging reads (3dworld_amd/csrc/terra_common.hpp: sg_chunk_len, sg_chunk_last_row, sg_last_row_read, SG_TABLE_ROWS),
// for every start term 0..90 and every chunk length the options allow.  The kernel's staging is replayed literally on a heap table of exactly SG_TABLE_ROWS rows and an
// "LDS" of exactly KC + 2 rows -- wave w copies the row pairs 2 w, 2 w + 8, ... below kn, as terra_kernels.hpp does -- so that the address sanitizer sees a row too many on
// either side, and the rows a sum uses are compared with the table's.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_sine_grid_paths_emul.py; exit status 0 = every check held.
#include "../../3dworld_amd/csrc/terra_common.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int failures = 0;
#define CHECK(cond) do {if (!(cond)) {fprintf(stderr, "%s:%d: CHECK(%s) failed (kstart %d, KC %d)\n", __FILE__, __LINE__, #cond, kstart, KC); ++failures;}} while (0)

int main() {
	using namespace terra;
	int const kcs[3] = {20, 27, 45};
	int const row_len = 128; // one block's slice of a table row
	for (int KC : kcs) {
		for (int kstart = 0; kstart <= F_TABLE_SIZE; ++kstart) {
			// a table as the driver allocates and fills it: rows kstart .. SG_TABLE_ROWS - 1 written (zeros behind row 89), the rows in front of kstart never touched
			std::vector<float> table((size_t)SG_TABLE_ROWS*row_len);
			for (int k = kstart; k < SG_TABLE_ROWS; ++k) {for (int x = 0; x < row_len; ++x) {table[(size_t)k*row_len + x] = (k < F_TABLE_SIZE) ? (float)(1000*k + x) : 0.0f;}}
			float *const lds = (float *)malloc((size_t)(KC + 2)*row_len*sizeof(float)); // (malloc: uninitialised, exactly KC + 2 rows)
			int const nk = F_TABLE_SIZE - kstart, nchunks = (nk + KC - 1)/KC, per_chunk = sg_chunk_len(kstart, KC);
			int last_read = -1, summed = 0;
			CHECK(per_chunk <= KC);
			for (int c = 0; c < nchunks; ++c) {
				int const k0 = kstart + c*per_chunk, kn = (k0 + per_chunk > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per_chunk;
				CHECK(kn > 0 && kn <= KC);
				for (int w = 0; w < 4; ++w) { // the four waves of a block
					for (int r = 2*w; r < kn; r += 8) {
						for (int lane = 0; lane < 64; ++lane) { // 16 bytes per lane: lanes 0..31 row r, lanes 32..63 row r + 1
							int const row = k0 + r + (lane >> 5);
							CHECK(row >= kstart && row < SG_TABLE_ROWS);
							CHECK(r + (lane >> 5) < KC + 2 - 1); // (the last LDS row is kept for the island terms)
							for (int j = 0; j < 4; ++j) {lds[(size_t)r*row_len + lane*4 + j] = table[(size_t)row*row_len + (lane & 31)*4 + j];}
							if (row > last_read) {last_read = row;}
						}
					}
				}
				CHECK(sg_chunk_last_row(k0, kn) <= sg_last_row_read(kstart, KC));
				for (int k = 0; k < kn; ++k, ++summed) { // the rows the sum uses hold the table's terms k0 .. k0 + kn - 1
					for (int x = 0; x < row_len; x += 37) {CHECK(lds[(size_t)k*row_len + x] == (float)(1000*(k0 + k) + x));}
				}
				if (kn & 1) {for (int x = 0; x < row_len; x += 37) {float const v = lds[(size_t)kn*row_len + x]; CHECK(v == v);}} // the extra row of an odd chunk: a table row, never a stray bit pattern
			}
			CHECK(summed == nk);
			CHECK(last_read == sg_last_row_read(kstart, KC));
			CHECK(sg_last_row_read(kstart, KC) < SG_TABLE_ROWS);
			free(lds);
		}
	}
	if (failures) {fprintf(stderr, "%d checks failed\n", failures); return 1;}
	printf("sg_table_rows_main: ok\n");
	return 0;
}
