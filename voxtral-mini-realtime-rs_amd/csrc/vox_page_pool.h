// The page allocator of a paged stream group (vox_stream_group_create_paged; DESIGN.md section 8, "Paged decoder cache"): host arithmetic alone, no device call --
// the free stack, every member's table mirror, the planning count and the release rule.  vox_api.cpp drives it and uploads the table entries it changes;
// tools/page_pool_check.cpp drives it alone (a randomised sequence under the host sanitizers).
//
// A member at decoder position P (its next tick) has written cache rows 0 .. P-1 and its next tick attends rows max(0, P - window) .. P.  Logical page q holds rows
// q * page_rows .. (q + 1) * page_rows - 1.  The member HOLDS the logical pages [first, end): end = ceil(P / page_rows) once the ticks up to P have their pages,
// first = max(0, P - window) / page_rows after the release that follows a committed call (window < 0: no window, nothing falls out).
//
// Two table forms.  BOUNDED (init): a member's table has one entry per logical page up to its position limit, tab[q].  RING (init_ring: an endless paged group, DESIGN.md
// section 8 "Endless paged groups"): the table has L = pool_pages entries and logical page q lives at tab[q % L].  A member never holds more pages than the pool has, so
// its held pages [first, end) -- at most L consecutive numbers -- never collide in the ring, whatever L is (no power of two needed); first and end run on as 64-bit
// logical page numbers.  A take that would make a member hold more than L pages would need more pages than the pool HAS, so it is the pool refusal itself (need >
// n_free): take() still checks it by name and refuses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

static const int PAGE_ROWS_MIN = 16, PAGE_ROWS_MAX = 1024, PAGE_ROWS_DEFAULT = 256;
inline bool page_rows_ok(int page_rows) { return page_rows >= PAGE_ROWS_MIN && page_rows <= PAGE_ROWS_MAX && (page_rows & (page_rows - 1)) == 0; }
// the logical pages a member at `positions` holds: [*first, *first + *n).  The one function behind vox_stream_group_pages_for, the planning and the release
inline void pages_held(int64_t positions, int page_rows, int window, int* first, int* n) {
    const int64_t lo = window >= 0 && positions > window ? positions - window : 0;
    *first = (int)(lo / page_rows);
    *n = (int)((positions + page_rows - 1) / page_rows) - *first;
}
struct PagePool {
    int page_rows = 0, shift = 0, window = -1, pool_pages = 0, max_pages = 0, peak = 0;      // max_pages: the logical pages of the position limit (both forms)
    bool ring = false; int tab_len = 0;      // entries of a member's table: max_pages (bounded), pool_pages (ring)
    std::vector<int> free_;                                           // the free physical pages, a LIFO stack: back() is taken next
    struct Member { std::vector<int> tab; int64_t first = 0, end = 0; };  // tab[slot(q)]: the physical page of logical page q, -1 where none is held; held: [first, end)
    std::vector<Member> mem;
    // what a peek takes back: the members' ends and the peak (nothing is released inside a peek, so the stack below the taken pages is untouched)
    struct Mark { std::vector<int64_t> end; int peak; };

    void init(int n_members, int page_rows_, int window_, int pool_pages_, int max_positions) {
        page_rows = page_rows_; window = window_; pool_pages = pool_pages_; peak = 0;
        shift = 0; while ((1 << shift) < page_rows) shift++;
        max_pages = (max_positions + page_rows - 1) / page_rows; ring = false; tab_len = max_pages;
        free_.resize((size_t)pool_pages);
        for (int i = 0; i < pool_pages; i++) free_[(size_t)i] = pool_pages - 1 - i;      // page 0 is taken first
        mem.assign((size_t)n_members, Member{});
        for (Member& m : mem) m.tab.assign((size_t)tab_len, -1);
    }
    // the ring form: tables of pool_pages entries, positions up to pos_limit
    void init_ring(int n_members, int page_rows_, int window_, int pool_pages_, int64_t pos_limit) {
        init(n_members, page_rows_, window_, pool_pages_, 0);
        max_pages = (int)((pos_limit + page_rows - 1) / page_rows); ring = true; tab_len = pool_pages;
        for (Member& m : mem) m.tab.assign((size_t)tab_len, -1);
    }
    size_t slot(int64_t q) const { return (size_t)(ring ? q % tab_len : q); }      // where logical page q lives in a member's table
    int at(int member, int64_t q) const { return mem[(size_t)member].tab[slot(q)]; }
    int n_free() const { return (int)free_.size(); }
    int held(int member) const { return (int)(mem[(size_t)member].end - mem[(size_t)member].first); }
    // pages the ticks up to position `target` enter beyond the ones the member holds (planning: nothing changes)
    int need(int member, int64_t target) const {
        int first, n; pages_held(target, page_rows, -1, &first, &n);
        return n > mem[(size_t)member].end ? (int)(n - mem[(size_t)member].end) : 0;
    }
    // takes them: false (nothing changed) when the pool has fewer free.  The new entries are tab[*q0 .. *q1 - 1]
    bool take(int member, int64_t target, int64_t* q0, int64_t* q1) {
        Member& m = mem[(size_t)member]; const int k = need(member, target);
        *q0 = m.end; *q1 = m.end + k;
        if (k > n_free() || m.end + k > max_pages) { *q1 = *q0; return false; }
        if (ring && m.end + k - m.first > tab_len) { *q1 = *q0; return false; }      // (never alone: held + free <= pool_pages = tab_len, so k > n_free above)
        for (int64_t q = m.end; q < m.end + k; q++) { m.tab[slot(q)] = free_.back(); free_.pop_back(); }
        m.end += k;
        if (pool_pages - n_free() > peak) peak = pool_pages - n_free();
        return true;
    }
    // after a committed call that left the member at position `pos`: the pages below its window go back.  The entries that became -1 are tab[*q0 .. *q1 - 1]
    void release_below_window(int member, int64_t pos, int64_t* q0, int64_t* q1) {
        Member& m = mem[(size_t)member]; int first_, n; pages_held(pos, page_rows, window, &first_, &n);
        int64_t first = first_;
        *q0 = m.first; *q1 = m.first;
        if (first > m.end) first = m.end;
        for (int64_t q = m.first; q < first; q++) { free_.push_back(m.tab[slot(q)]); m.tab[slot(q)] = -1; }
        if (first > m.first) { *q1 = first; m.first = first; }
    }
    // reset: every page of the member goes back (the caller then takes the seed's).  The entries that became -1 are tab[*q0 .. *q1 - 1]
    void release_all(int member, int64_t* q0, int64_t* q1) {
        Member& m = mem[(size_t)member]; *q0 = m.first; *q1 = m.end;
        for (int64_t q = m.first; q < m.end; q++) { free_.push_back(m.tab[slot(q)]); m.tab[slot(q)] = -1; }
        m.first = m.end = 0;
    }
    // restore (vox_stream_group_restore): a member that holds nothing (release_all) starts at logical page q -- the first page of the window it is about to take
    void start_at(int member, int64_t q) { Member& m = mem[(size_t)member]; if (m.first == m.end) m.first = m.end = q; }
    Mark mark() const { Mark k; k.peak = peak; for (const Member& m : mem) k.end.push_back(m.end); return k; }
    // the pages taken since the mark go back in the reverse order of their taking, last member first: the stack, the tables and the peak are what they were,
    // PROVIDED the members took their pages in ascending member-slot order `order` (the order given here) and nothing was released in between
    void undo(const Mark& k, const std::vector<int>& order) {
        for (size_t z = order.size(); z-- > 0;) {
            Member& m = mem[(size_t)order[z]];
            for (int64_t q = m.end; q-- > k.end[(size_t)order[z]];) { free_.push_back(m.tab[slot(q)]); m.tab[slot(q)] = -1; }
            m.end = k.end[(size_t)order[z]];
        }
        peak = k.peak;
    }
    // every page is on the stack or in exactly one table, the held ranges are the only entries >= 0
    bool consistent() const {
        std::vector<char> seen((size_t)pool_pages, 0); int total = 0;
        for (int p : free_) { if (p < 0 || p >= pool_pages || seen[(size_t)p]) return false; seen[(size_t)p] = 1; total++; }
        for (const Member& m : mem) {
            if (m.first < 0 || m.first > m.end || m.end > max_pages || m.end - m.first > tab_len || (int)m.tab.size() != tab_len) return false;
            for (int q = 0; q < tab_len; q++) {      // (ring: entry q is held when it lies less than `held` entries behind first's)
                const int p = m.tab[(size_t)q];
                const bool in = ring ? (q - (int)(m.first % tab_len) + tab_len) % tab_len < m.end - m.first : q >= m.first && q < m.end;
                if (in != (p >= 0)) return false;
                if (in) { if (p >= pool_pages || seen[(size_t)p]) return false; seen[(size_t)p] = 1; total++; }
            }
        }
        return total == pool_pages;
    }
};
