// rtw_plain_layout.hpp -- which spheres share a block of 32 in the plain matrix-pipe scan (hit_world_mfma without the vote), built on the host.
// Plain C++ (no HIP): rtw_scene.hip uploads the arrays in this order, tests/plain_layout_check.cpp checks it on the CPU.
// The scan tests every sphere against every ray whatever the order; what the order decides is how often a (wave, block) evaluation finds
// no candidate in any lane and skips the sign collection, the entry record and its share of pass 2.  Rays of a wave are neighbours, so a
// block whose spheres are neighbours is skipped more often than 32 consecutive spheres of the caller's list (for the reference's scene a
// row and a half of the lattice).
#pragma once
#include <algorithm>
#include <vector>

#define RTW_PLAIN_BLOCK 32

namespace rtwh {

struct PlainLayout {
    int blocks = 0;            // ceil(n / 32): never more than the caller's order needs
    std::vector<int> slot;     // blocks x 32 entries: the input sphere in that row of the operand blocks, -1 = unused row (a dead sphere)
};

// cx / cy / cz: the centres of the n spheres that go through the filter, in the caller's order.  The set is split into `blocks` leaves by
// kd median splits on the widest axis of the centres; a node of L leaves hands floor(L / 2) of them to its lower side, and the spheres are
// dealt so that the leaf sizes differ by at most one (n = 484: 16 leaves of 30 or 31, not 15 full blocks and a tail of 4).  Leaf k is
// block k, its spheres in the caller's order.  Ties: spheres are ordered by (coordinate, input index) and the first of equally wide axes
// is taken, so the same input always gives the same permutation.  At most one block: the caller's order.
inline void build_plain_layout(const double *cx, const double *cy, const double *cz, int n, PlainLayout *out) {
    constexpr int B = RTW_PLAIN_BLOCK;
    out->blocks = n > 0 ? (n + B - 1) / B : 0;
    out->slot.assign((size_t)out->blocks * B, -1);
    if (out->blocks <= 1) {
        for (int i = 0; i < n; ++i) out->slot[i] = i;
        return;
    }
    std::vector<int> ids(n);
    for (int i = 0; i < n; ++i) ids[i] = i;
    const double *c[3] = {cx, cy, cz};
    struct Node { int lo, hi, leaf0, leaves; };
    std::vector<Node> todo;
    todo.push_back(Node{0, n, 0, out->blocks});
    while (!todo.empty()) {
        const Node nd = todo.back();
        todo.pop_back();
        const int cnt = nd.hi - nd.lo;
        if (nd.leaves == 1) {
            std::sort(ids.begin() + nd.lo, ids.begin() + nd.hi);
            for (int k = 0; k < cnt; ++k) out->slot[(size_t)nd.leaf0 * B + k] = ids[nd.lo + k];
            continue;
        }
        int ax = 0;
        double ext[3];
        for (int a = 0; a < 3; ++a) {
            double mn = c[a][ids[nd.lo]], mx = mn;
            for (int k = nd.lo + 1; k < nd.hi; ++k) { mn = std::min(mn, c[a][ids[k]]); mx = std::max(mx, c[a][ids[k]]); }
            ext[a] = mx - mn;
        }
        for (int a = 1; a < 3; ++a) if (ext[a] > ext[ax]) ax = a;
        const double *key = c[ax];
        std::sort(ids.begin() + nd.lo, ids.begin() + nd.hi, [key](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
        // cnt = leaves x base + rem: `rem` leaves hold base + 1 spheres; the lower side takes its leaves' share of both kinds
        const int base = cnt / nd.leaves, rem = cnt % nd.leaves, left = nd.leaves / 2;
        const int left_cnt = left * base + std::min(rem, left);
        todo.push_back(Node{nd.lo, nd.lo + left_cnt, nd.leaf0, left});
        todo.push_back(Node{nd.lo + left_cnt, nd.hi, nd.leaf0 + left, nd.leaves - left});
    }
}

}  // namespace rtwh
