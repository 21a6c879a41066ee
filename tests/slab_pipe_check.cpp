// Stand-alone check of wtp::run_slabs (csrc/wtp_slab_pipe.hpp), built and run by
// tests/test_slab_pipe.py.  Arguments come in fours: n per fail_issue fail_retire, where
// fail_x = k > 0 makes the k-th call of x return 7 (issue) or 9 (retire).  One line per case:
// the calls in order, as I<buffer>[<first>+<count>] / R<buffer>[<first>+<count>], then rc.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "wtp_slab_pipe.hpp"

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 1) % 4 != 0) return 2;
    for (int a = 1; a < argc; a += 4) {
        const size_t n = strtoull(argv[a], nullptr, 10), per = strtoull(argv[a + 1], nullptr, 10);
        const long fail_issue = atol(argv[a + 2]), fail_retire = atol(argv[a + 3]);
        std::string log;
        long issued = 0, retired = 0;
        auto event = [&](char what, int b, size_t first, size_t count) {
            log += (log.empty() ? "" : " ") + std::string(1, what) + std::to_string(b) + "[" + std::to_string(first) + "+" +
                   std::to_string(count) + "]";
        };
        const int rc = wtp::run_slabs(
            n, per,
            [&](int b, size_t first, size_t count) {
                event('I', b, first, count);
                return ++issued == fail_issue ? 7 : 0;
            },
            [&](int b, size_t first, size_t count) {
                event('R', b, first, count);
                return ++retired == fail_retire ? 9 : 0;
            });
        std::printf("%s|rc=%d\n", log.c_str(), rc);
    }
    return 0;
}
