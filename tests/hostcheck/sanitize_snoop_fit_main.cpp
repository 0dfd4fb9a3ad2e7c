// Stand-alone driver of the scratch layouts behind vba_snoop_scaled (vinsat_amd/csrc/vba_query_layout.h) for an AddressSanitizer /
// UBSan build on the CPU (tests/test_snoop_scaled_host.py): the query's own scratch (snoop_fit_layout: three doubles per pose, two
// per window) and the snoop state it sits beside (snoop_layout, unchanged), at the smallest shape and at one that is no multiple
// of anything.  Counted and then placed over a block of the counted size: the buffers come in order, each on a multiple of 256
// bytes, the last one ends inside the block, counted size equals placed size.  Every buffer is written over its whole length, so
// an overrun is the sanitizer's to report.
#include "../../vinsat_amd/csrc/vba_query_layout.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Span { void* p; size_t bytes; };
static int check_spans(char* base, size_t total, const std::vector<Span>& spans) {
    int bad = 0;
    const char* end_prev = base;
    for (const Span& sp : spans) {
        const char* p = static_cast<const char*>(sp.p);
        if (p < end_prev || (reinterpret_cast<uintptr_t>(p) & 255u) != 0 || p + sp.bytes > base + total) ++bad;
        else std::memset(sp.p, 0x5a, sp.bytes);
        end_prev = p + sp.bytes;
    }
    return bad;
}

static int check_layouts(size_t W, size_t N, size_t M) {
    int bad = 0;
    {
        Carver count;
        snoop_fit_layout(count, W, N);
        if (count.total() < (W * N * 3 + W * 2) * 8) ++bad;
        char* base = static_cast<char*>(std::aligned_alloc(256, count.total()));
        Carver place{base};
        const SnoopFitBufs b = snoop_fit_layout(place, W, N);
        if (place.total() != count.total()) ++bad;
        if (static_cast<void*>(b.pose) != static_cast<void*>(base)) ++bad;
        bad += check_spans(base, count.total(), {{b.pose, W * N * 3 * 8}, {b.win, W * 2 * 8}});
        std::free(base);
    }
    {
        Carver count;
        snoop_layout(count, W, N, M);
        char* base = static_cast<char*>(std::aligned_alloc(256, count.total()));
        Carver place{base};
        const SnoopBufs b = snoop_layout(place, W, N, M);
        if (place.total() != count.total()) ++bad;
        bad += check_spans(base, count.total(), {{b.orig, W * M * 8}, {b.mask, W * M}, {b.prej, W * N * 4}});
        std::free(base);
    }
    return bad;
}

int main() {
    const int bad = check_layouts(1, 2, 3) + check_layouts(3, 17, 67);
    if (bad) { std::printf("sanitize_snoop_fit_main: %d failures\n", bad); return 1; }
    std::printf("sanitize_snoop_fit_main ok\n");
    return 0;
}
