// obs_split (csrc/mev_obs_chunks.h), exhaustively: for every base phase, row stride, beam
// count, row and slice start the kernel can meet, replaying the stores the kernel derives
// from it writes every float of the slice exactly once -- by a 16-byte aligned chunk lying
// wholly inside the slice or by a single-float store -- and touches no byte outside it.
// The rows live in a heap block of exactly their size, so a sanitized build of this
// program also traps any store past either end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mev_obs_chunks.h"

using mev::ObsSplit;

static long g_fail = 0;
static void fail(const char* what, int phase, int ld, int ls, int row, int start) {
    if (g_fail++ < 20) printf("FAIL %s: phase %d obs_ld %d LS %d row %d start %d\n", what, phase, ld, ls, row, start);
}

int main() {
    const int ROWS = 16, HEAD = 31;
    long cases = 0, chunks = 0, singles = 0;
    for (int phase = 0; phase < 4; ++phase)
        for (int ls = 1; ls <= 128; ++ls)
            for (int ld = HEAD + ls; ld <= HEAD + ls + 40; ++ld) {
                const size_t n = (size_t)ROWS * ld;
                void* raw = nullptr;
                if (posix_memalign(&raw, 16, (n + phase) * sizeof(uint32_t)) != 0) return 2;
                uint32_t* base = (uint32_t*)raw + phase;  // `phase` floats past a 16-byte boundary
                for (int start = 0; start <= HEAD; start += HEAD) {  // the head [0, 31) and the LiDAR block
                    const int len = start == 0 ? HEAD : ls;
                    for (int row = 0; row < ROWS; ++row) {
                        ++cases;
                        // (the stores below are checked against the slice before they are made, so
                        // the exactly-once scan needs the slice and a margin, not all 16 rows)
                        const size_t lo = (size_t)row * ld + start, hi = lo + len;
                        const size_t w0 = lo > 16 ? lo - 16 : 0, w1 = hi + 16 < n ? hi + 16 : n;
                        for (size_t i = w0; i < w1; ++i) base[i] = 0;
                        uint32_t* slice = base + lo;
                        const ObsSplit s = mev::obs_split((uint64_t)(uintptr_t)slice, len);
                        if (s.prefix < 0 || s.prefix > 3 || s.suffix < 0 || s.suffix > 3 || s.chunks < 0 ||
                            s.prefix + 4 * s.chunks + s.suffix != len)
                            fail("shape", phase, ld, ls, row, start);
                        for (int c = 0; c < s.chunks; ++c) {  // a lane's 16-byte store
                            uint32_t* q = slice + s.prefix + 4 * c;
                            if (((uintptr_t)q & 15) != 0) fail("chunk not 16-byte aligned", phase, ld, ls, row, start);
                            if (q < slice || q + 4 > slice + len) {
                                fail("chunk outside the slice", phase, ld, ls, row, start);
                                continue;
                            }
                            for (int i = 0; i < 4; ++i) q[i] += 1;
                            ++chunks;
                        }
                        for (int slot = 0; slot < 8; ++slot) {  // the single-float pass: 8 lanes per row
                            const int b = slot < 6 ? mev::obs_split_single(s, slot) : -1;
                            if (b < 0) continue;
                            if (b >= len) {
                                fail("single outside the slice", phase, ld, ls, row, start);
                                continue;
                            }
                            slice[b] += 1;
                            ++singles;
                        }
                        for (size_t i = w0; i < w1; ++i)
                            if (base[i] != (i >= lo && i < hi ? 1u : 0u)) {
                                fail(i >= lo && i < hi ? "float not written exactly once" : "write outside the slice",
                                     phase, ld, ls, row, start);
                                break;
                            }
                    }
                }
                free(raw);
            }
    printf("%ld cases, %ld chunks, %ld single floats, %ld failures\n", cases, chunks, singles, g_fail);
    if (g_fail) return 1;
    printf("OBS CHUNKS OK\n");
    return 0;
}
