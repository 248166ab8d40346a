// Termination and coverage of the leaf cursor (csrc/leaf_cursor.h), exhaustively on the CPU: every first in [0, 2^20), count 1..4,
// K in {1, 2}. Built with -fsanitize=address,undefined by tests/test_leaf_cursor_host.py; a stand-alone program.
#include "../gradient-based-path-tracing_amd/csrc/leaf_cursor.h"

#include <climits>
#include <cstdio>

static const int kTravDone = INT_MIN;    // render_device.h

static int fail(const char *what, unsigned first, unsigned count, int K, int cur) {
    std::printf("leaf_cursor_check FAILED: %s (first %u count %u K %d cur %d)\n", what, first, count, K, cur);
    return 1;
}

int main() {
    unsigned long long steps_total = 0;
    for (int K = 1; K <= 2; K++)
        for (unsigned count = 1; count <= 4; count++)
            for (unsigned first = 0; first < (1u << 20); first++) {
                int cur = (int)~((first << 2) | (count - 1u));
                unsigned next_record = first, remaining = count, steps = 0;
                for (;;) {
                    if (cur >= 0) return fail("value >= 0", first, count, K, cur);
                    if (cur == kTravDone) return fail("value equals kTravDone", first, count, K, cur);
                    const unsigned packed = ~(unsigned)cur, f = packed >> 2, c = (packed & 3u) + 1u;
                    if (f != next_record) return fail("leaf does not start at the next untested record", first, count, K, cur);
                    if (c != remaining) return fail("wrong remaining count", first, count, K, cur);
                    // the step tests records f .. f + n - 1
                    const unsigned n = gd::leaf_step_records(cur, K);
                    if (n != (c < (unsigned)K ? c : (unsigned)K) || n == 0) return fail("records per step", first, count, K, cur);
                    next_record += n;
                    steps++;
                    const int before = cur;
                    const bool more = gd::leaf_advance(cur, K);
                    if (!more) {
                        if (cur != before) return fail("pop changed cur", first, count, K, cur);
                        if (n != remaining) return fail("pop with records left", first, count, K, cur);
                        remaining = 0;
                        break;
                    }
                    if (n != (unsigned)K) return fail("advance after a short step", first, count, K, cur);
                    const unsigned left = (~(unsigned)cur & 3u) + 1u;
                    if (!(left < remaining)) return fail("remaining count did not fall", first, count, K, cur);
                    remaining -= n;
                    if (steps > 4) return fail("more than four steps", first, count, K, cur);
                }
                if (next_record != first + count) return fail("records visited != first .. first + count - 1", first, count, K, cur);
                if (steps != (count + (unsigned)K - 1u) / (unsigned)K) return fail("steps != ceil(count / K)", first, count, K, cur);
                steps_total += steps;
            }
    std::printf("leaf_cursor_check ok (%llu steps)\n", steps_total);
    return 0;
}
