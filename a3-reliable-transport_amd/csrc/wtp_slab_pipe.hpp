// wtp_slab_pipe.hpp — the two-buffer pipeline of the host-memory calls (wtp_host.cpp), as
// bookkeeping alone: no HIP header, no HIP call, so a plain C++ program can check it
// (tests/slab_pipe_check.cpp).  Internal: the C-ABI is include/wtp_crc32.h.
#pragma once
#include <algorithm>
#include <cstddef>

namespace wtp {

// Items [0, n) in slabs of `per`, slab k on buffer/stream k % 2, two slabs in flight:
//   issue(b, first, count) -> rc    stage + H2D + launches + D2H of items [first, first + count)
//   retire(b, first, count) -> rc   wait for stream b, copy that slab's results out
// A slab is retired just before its buffer is issued again, and the last two at the end:
// I0 I1 R0 I2 R1 I3 ... R(k-2) R(k-1).  A non-zero rc is returned at once, with nothing more
// issued and no live slab retired: the caller drains both streams.  per == 0 with items to
// run is a mistake in the caller, which must make it impossible (wtp_host.cpp's slab sizes
// are at least 1) and not pass it on: a bare -1, no WTP_* code or message, nothing called.
template <class Issue, class Retire>
int run_slabs(size_t n, size_t per, Issue issue, Retire retire) {
    if (per == 0) return n ? -1 : 0;
    const size_t slabs = n / per + (n % per != 0);
    auto count = [&](size_t k) { return std::min(per, n - k * per); };
    for (size_t k = 0; k < slabs + 2; ++k) {
        if (k >= 2)
            if (int rc = retire(int(k & 1), (k - 2) * per, count(k - 2))) return rc;
        if (k < slabs)
            if (int rc = issue(int(k & 1), k * per, count(k))) return rc;
    }
    return 0;
}

}  // namespace wtp
