// The paged stream group's allocator (csrc/vox_page_pool.h) on its own: a randomised sequence of the four things the group does with it -- a committed call (plan, take,
// release below the window), a refused call (plan alone), a reset (release all, take the seed) and a peek (mark, take, undo) -- checked after every step against a
// plain model (a set of free pages, a map per member) and against the allocator's own consistency check.  Every run is one of the two table forms: the bounded table
// (one entry per logical page up to max_positions) or the RING table of an endless group (pool_pages entries, logical page q at entry q % pool_pages), whose members
// start at large logical page numbers -- as sessions far into their run -- so that the page numbers run far past the table's length and wrap it many times; a ring
// run's members go on to 2^24 positions.  Host code only, no device call: build it with the host
// sanitizers and run it on the CPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I voxtral-mini-realtime-rs_amd/csrc tools/page_pool_check.cpp -o page_pool_check && ./page_pool_check
#include "vox_page_pool.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "page_pool_check: %s failed at line %d (seed %u, step %d)\n", #cond, __LINE__, seed, step); return 1; } } while (0)

static unsigned seed = 0; static int step = 0;

static int run(unsigned sd, int steps, bool ring) {
    seed = sd; std::mt19937 rng(sd);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    const int page_rows = 16 << pick(0, 6), n = pick(1, 16), PC = 37, max_pos = ring ? 1 << 24 : pick(PC + 1, 16384);
    const int window = !ring && pick(0, 3) == 0 ? -1 : pick(1, 9000);      // (an endless group has a window)
    const int seed_pages = (PC + page_rows - 1) / page_rows, most = (max_pos + page_rows - 1) / page_rows;
    // ring: from the seeds alone to a pool in which every member holds a window and a call's pages at once
    const int pool_pages = ring ? pick(n * seed_pages, n * (window / page_rows + 6)) : pick(n * seed_pages, n * most);
    PagePool pool; if (ring) pool.init_ring(n, page_rows, window, pool_pages, max_pos); else pool.init(n, page_rows, window, pool_pages, max_pos);
    CHECK(pool.tab_len == (ring ? pool_pages : most));
    std::vector<int> pos((size_t)n, PC), base((size_t)n, 0);      // base: the logical page a rebased member started at (it never held the pages below)
    // the model: which physical page holds logical page q of member i
    std::vector<std::map<int64_t, int>> own((size_t)n); std::set<int> free_;
    for (int p = 0; p < pool_pages; p++) free_.insert(p);
    auto agree = [&]() -> bool {
        if (!pool.consistent() || pool.n_free() != (int)free_.size()) return false;
        for (int p : pool.free_) if (!free_.count(p)) return false;
        for (int i = 0; i < n; i++) {
            const PagePool::Member& m = pool.mem[(size_t)i];
            if ((int64_t)own[(size_t)i].size() != m.end - m.first || (int)own[(size_t)i].size() > pool.tab_len) return false;
            for (const auto& kv : own[(size_t)i]) if (kv.first < m.first || kv.first >= m.end || pool.at(i, kv.first) != kv.second) return false;
        }
        return true;
    };
    auto model_take = [&](int i, int64_t q0, int64_t q1) { for (int64_t q = q0; q < q1; q++) { const int p = pool.at(i, q); if (!free_.erase(p)) return false; own[(size_t)i][q] = p; } return true; };
    for (int i = 0; i < n; i++) { int64_t q0, q1; CHECK(pool.take(i, PC, &q0, &q1)); CHECK(q0 == 0 && q1 == seed_pages); CHECK(model_take(i, q0, q1)); }
    CHECK(agree()); CHECK(pool.peak == n * seed_pages);
    if (ring) {      // most members go on as sessions far into their run: logical page numbers far past the table's length, some just below the position limit
        for (int i = 0; i < n; i++) {
            if (pick(0, 3) == 0) continue;
            const int at = pick(0, 2) == 0 ? max_pos - pick(1, 40 * page_rows) : pick(2 * pool_pages * page_rows, max_pos - 1), first = at / page_rows;
            if (first < seed_pages) continue;
            int64_t q0, q1; pool.release_all(i, &q0, &q1);
            for (const auto& kv : own[(size_t)i]) free_.insert(kv.second);
            own[(size_t)i].clear();
            pool.mem[(size_t)i].first = pool.mem[(size_t)i].end = first; /* it holds nothing: its held range is empty wherever it lies */ pos[(size_t)i] = first * page_rows; base[(size_t)i] = first;
            CHECK(pool.mem[(size_t)i].first == first && pool.held(i) == 0); CHECK(agree());
        }
    }
    for (step = 0; step < steps; step++) {
        const int what = pick(0, 9);
        if (what <= 5) {      // a call: a subset of members, each some ticks; planned first, all or nothing
            std::vector<int> who, target; int need = 0;
            for (int i = 0; i < n; i++) if (pick(0, 2) == 0 && pos[(size_t)i] < max_pos) { who.push_back(i); target.push_back(std::min(max_pos, pos[(size_t)i] + pick(0, 3 * page_rows))); }
            for (size_t z = 0; z < who.size(); z++) need += pool.need(who[z], target[z]);
            const int free_was = pool.n_free(), peak_was = pool.peak; const std::vector<int> stack_was = pool.free_;
            if (need > pool.n_free()) { CHECK(agree()); CHECK(pool.free_ == stack_was && pool.peak == peak_was); continue; }      // refused: nothing changed
            const bool peek = what == 5; const PagePool::Mark mk = pool.mark();
            std::vector<std::map<int64_t, int>> own_was = own; std::set<int> model_free_was = free_;
            for (size_t z = 0; z < who.size(); z++) {
                int64_t q0, q1; const int top = pool.n_free() ? pool.free_.back() : -1;
                CHECK(pool.take(who[z], target[z], &q0, &q1));
                if (q1 > q0) CHECK(pool.at(who[z], q0) == top);      // LIFO: the page on top goes first
                CHECK(model_take(who[z], q0, q1));
                CHECK(q1 == (target[z] + page_rows - 1) / page_rows || q1 == q0);
            }
            CHECK(pool.n_free() == free_was - need); CHECK(agree());
            if (peek) {      // taken back: the stack, the tables and the peak are what they were
                pool.undo(mk, who); own = own_was; free_ = model_free_was;
                CHECK(pool.free_ == stack_was && pool.peak == peak_was); CHECK(agree());
                continue;
            }
            CHECK(pool.peak == std::max(peak_was, pool_pages - pool.n_free()));
            for (size_t z = 0; z < who.size(); z++) {      // committed: the positions move, the pages below the window go back
                const int i = who[z]; pos[(size_t)i] = target[z];
                int64_t q0, q1; pool.release_below_window(i, pos[(size_t)i], &q0, &q1);
                for (int64_t q = q0; q < q1; q++) { CHECK(own[(size_t)i].count(q)); free_.insert(own[(size_t)i][q]); own[(size_t)i].erase(q); }
                int first, cnt; pages_held(pos[(size_t)i], page_rows, window, &first, &cnt);
                const int lo = std::max(first, base[(size_t)i]);      // what the member holds is what pages_held says (a rebased member: from its start on)
                CHECK(pool.mem[(size_t)i].first == lo && pool.held(i) == first + cnt - lo);
                const int j_lo = window >= 0 && pos[(size_t)i] > window ? pos[(size_t)i] - window : 0;      // every row its next tick attends lies in a held page
                for (int j : {j_lo, pos[(size_t)i] - 1}) if (j >= 0 && j < pos[(size_t)i] && j / page_rows >= pool.mem[(size_t)i].first) CHECK(pool.at(i, j / page_rows) >= 0);
            }
            CHECK(agree());
        } else {      // a reset
            const int i = pick(0, n - 1); int64_t q0, q1, t0, t1;
            if (pool.held(i) + pool.n_free() < seed_pages) continue;      // (a short window on a full pool: the group refuses this reset)
            pool.release_all(i, &q0, &q1);
            for (const auto& kv : own[(size_t)i]) free_.insert(kv.second);
            own[(size_t)i].clear();
            CHECK(pool.take(i, PC, &t0, &t1)); CHECK(t0 == 0 && t1 == seed_pages); CHECK(model_take(i, t0, t1));
            pos[(size_t)i] = PC; base[(size_t)i] = 0; CHECK(agree());
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const int runs = argc > 1 ? std::atoi(argv[1]) : 200, steps = argc > 2 ? std::atoi(argv[2]) : 400;
    for (int r = 0; r < runs; r++) if (run(1000u + (unsigned)r, steps, false)) return 1;
    for (int r = 0; r < runs; r++) if (run(5000u + (unsigned)r, steps, true)) return 1;
    std::printf("page_pool_check: %d bounded and %d ring runs of %d steps ok\n", runs, runs, steps);
    return 0;
}
