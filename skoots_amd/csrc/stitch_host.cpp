// The greedy stitch of skoots/utils/flood_and_stitch.py:74-128, played on component tables (plain C++, no GPU calls).
//
// The reference renames voxels: for every slice i and every label u of slice i-1 it picks the label of slice i that
// overlaps u most, then writes a new id over u in ALL slices before i and over the chosen label in slice i.  No voxel
// is needed for that.  A component of the plane labelling never splits, so the state is one label per component, and
// the overlaps of adjacent planes' components (sk_plane_overlaps) never change.  What changes is which components carry
// the same number, and that is a partition:
//
//   - every component belongs to a group (union-find, the group's current label kept at its root);
//   - the slices before i are ONE region, a hash map label -> group.  "Rename u in all slices before i" moves that one
//     group to the new key, or merges it into the group that already has the key: O(1), not a sweep;
//   - slice i has a map of its own until the walk has passed it, then its groups join the region's by label value;
//   - the components of slice i-1 read their current label through their group.
//
// Cost per pass: O(components + rows) map operations, whatever the number of renames.
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/skoots_hip.h"

namespace sk {
void set_error(const char* fmt, ...);
}

namespace {

struct Walk {
    int P;
    const int32_t* off;
    const int32_t* rows;
    int64_t n_rows;
    std::vector<int64_t> fwd_start;   // rows of id_a == c: [fwd_start[c], fwd_start[c + 1])
    std::vector<int64_t> rev_start;   // rev_rows of id_b == c
    std::vector<int64_t> rev_rows;    // row indices ordered by id_b
    std::vector<int32_t> cur;         // label of every component between the passes
    std::vector<int32_t> parent, lab, size;

    int find(int x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    }
    int unite(int a, int b) {   // roots in, root out
        if (a == b) return a;
        if (size[a] < size[b]) std::swap(a, b);
        parent[b] = a;
        size[a] += size[b];
        return a;
    }

    // key -> group with the label `to`; a group that already has `to` absorbs it.  Returns the group's root.
    int rename(std::unordered_map<int32_t, int>& map, int32_t from, int32_t to) {
        int r = find(map.at(from));
        map.erase(from);
        auto hit = map.find(to);
        if (hit != map.end()) r = unite(r, find(hit->second));
        lab[r] = to;
        map[to] = r;
        return r;
    }

    // one pass over the planes in the order first, first + step, ...; returns false when a new id would pass INT32_MAX
    bool pass(bool reverse) {
        const int T = off[P];
        for (int c = 1; c <= T; ++c) {
            parent[c] = c;
            size[c] = 1;
            lab[c] = cur[c];
        }
        int64_t newind = 0;
        for (int c = 1; c <= T; ++c) newind = std::max<int64_t>(newind, cur[c]);   // :75  the first new id EQUALS the maximum

        std::unordered_map<int32_t, int> region, slice;
        std::unordered_map<int, std::vector<int>> members;   // group root -> components of slice i-1
        std::vector<int32_t> ulist;
        std::vector<std::pair<int32_t, int64_t>> hits;

        auto group_plane = [&](int p, std::unordered_map<int32_t, int>& map) {   // components of one plane by label
            map.clear();
            for (int c = off[p] + 1; c <= off[p + 1]; ++c) {
                auto ins = map.emplace(lab[c], c);
                if (!ins.second) ins.first->second = unite(find(ins.first->second), c);
            }
        };
        auto join_region = [&](const std::unordered_map<int32_t, int>& map) {
            for (const auto& kv : map) {
                const int r = find(kv.second);
                auto ins = region.emplace(kv.first, r);
                if (!ins.second) ins.first->second = unite(find(ins.first->second), r);
            }
        };

        const int first = reverse ? P - 1 : 0, step = reverse ? -1 : 1;
        group_plane(first, slice);
        join_region(slice);
        for (int i = 1; i < P; ++i) {
            const int pa = first + (i - 1) * step, pb = first + i * step;
            group_plane(pb, slice);
            members.clear();
            for (int c = off[pa] + 1; c <= off[pa + 1]; ++c) members[find(c)].push_back(c);
            ulist.clear();
            for (const auto& kv : members) ulist.push_back(lab[kv.first]);   // one group per label in the region
            std::sort(ulist.begin(), ulist.end());                           // :85  np.unique, taken before the loop
            for (const int32_t u : ulist) {
                auto reg = region.find(u);
                if (reg == region.end()) continue;
                const int ru = find(reg->second);
                auto mem = members.find(ru);
                if (mem == members.end()) continue;
                hits.clear();
                for (const int c : mem->second) {
                    const int64_t lo = reverse ? rev_start[c] : fwd_start[c], hi = reverse ? rev_start[c + 1] : fwd_start[c + 1];
                    for (int64_t k = lo; k < hi; ++k) {
                        const int64_t row = reverse ? rev_rows[k] : k;
                        const int other = rows[3 * row + (reverse ? 0 : 1)];
                        const int32_t l = lab[find(other)];
                        if (l != u) hits.emplace_back(l, rows[3 * row + 2]);   // :100  a slice-i label equal to u is left out
                    }
                }
                if (hits.empty()) continue;
                std::sort(hits.begin(), hits.end());
                int32_t best = 0;
                int64_t best_n = -1;
                for (size_t k = 0; k < hits.size();) {   // :108  argmax over the sorted labels: ties go to the smallest
                    size_t e = k;
                    int64_t n = 0;
                    for (; e < hits.size() && hits[e].first == hits[k].first; ++e) n += hits[e].second;
                    if (n > best_n) {
                        best_n = n;
                        best = hits[k].first;
                    }
                    k = e;
                }
                if (newind > INT32_MAX) return false;
                const int32_t id = (int32_t)newind;
                // :120-121  u -> id in all slices before i: one group of the region moves, or merges into the key's owner
                auto other = region.find(id);
                const int absorbed = (other != region.end() && id != u) ? find(other->second) : -1;
                const int r = rename(region, u, id);
                std::vector<int> moved;
                for (const int old : {ru, absorbed}) {
                    if (old < 0 || old == r) continue;
                    auto m = members.find(old);
                    if (m == members.end()) continue;
                    moved.insert(moved.end(), m->second.begin(), m->second.end());
                    members.erase(m);
                }
                if (!moved.empty()) {
                    std::vector<int>& dst = members[r];
                    dst.insert(dst.end(), moved.begin(), moved.end());
                }
                rename(slice, best, id);   // :123  the chosen label of slice i
                ++newind;
            }
            join_region(slice);
        }
        for (int c = 1; c <= T; ++c) cur[c] = lab[find(c)];
        return true;
    }
};

}  // namespace

extern "C" int sk_stitch_walk_host(const int32_t* offsets_host, int n_planes, const int32_t* rows_host, int64_t n_rows,
                                   int32_t* lut_host, int32_t* max_label_host) {
    if (!offsets_host || !lut_host || !max_label_host || n_planes < 1 || n_rows < 0 || (n_rows > 0 && !rows_host)) {
        sk::set_error("sk_stitch_walk_host: bad arguments");
        return SK_ERR_ARG;
    }
    if (offsets_host[0] != 0) {
        sk::set_error("sk_stitch_walk_host: offsets[0] = %d, not 0", offsets_host[0]);
        return SK_ERR_ARG;
    }
    for (int p = 0; p < n_planes; ++p)
        if (offsets_host[p + 1] < offsets_host[p] || offsets_host[p + 1] == INT32_MAX) {
            sk::set_error("sk_stitch_walk_host: offsets decrease or overflow at plane %d", p);
            return SK_ERR_ARG;
        }
    const int T = offsets_host[n_planes];
    Walk w;
    w.P = n_planes;
    w.off = offsets_host;
    w.rows = rows_host;
    w.n_rows = n_rows;
    std::vector<int> plane((size_t)T + 1, -1);
    for (int p = 0; p < n_planes; ++p)
        for (int c = offsets_host[p] + 1; c <= offsets_host[p + 1]; ++c) plane[c] = p;
    w.fwd_start.assign((size_t)T + 2, 0);
    w.rev_start.assign((size_t)T + 2, 0);
    for (int64_t k = 0; k < n_rows; ++k) {
        const int32_t a = rows_host[3 * k], b = rows_host[3 * k + 1], n = rows_host[3 * k + 2];
        const bool ok = a >= 1 && a <= T && b >= 1 && b <= T && n > 0 && plane[b] == plane[a] + 1;
        const bool sorted = k == 0 || rows_host[3 * k - 3] < a || (rows_host[3 * k - 3] == a && rows_host[3 * k - 2] < b);
        if (!ok || !sorted) {
            sk::set_error("sk_stitch_walk_host: row %lld (%d, %d, %d) is out of range, not between adjacent planes, or not in "
                          "(id_a, id_b) order", (long long)k, a, b, n);
            return SK_ERR_ARG;
        }
        ++w.fwd_start[a + 1];
        ++w.rev_start[b + 1];
    }
    for (int c = 1; c <= T + 1; ++c) {
        w.fwd_start[c] += w.fwd_start[c - 1];
        w.rev_start[c] += w.rev_start[c - 1];
    }
    w.rev_rows.resize((size_t)n_rows);
    {
        std::vector<int64_t> fill(w.rev_start.begin(), w.rev_start.end());
        for (int64_t k = 0; k < n_rows; ++k) w.rev_rows[fill[rows_host[3 * k + 1]]++] = k;
    }
    w.cur.assign((size_t)T + 1, 0);
    for (int c = 1; c <= T; ++c) w.cur[c] = c - offsets_host[plane[c]];   // :63-69  numbering restarts in every slice
    w.parent.assign((size_t)T + 1, 0);
    w.lab.assign((size_t)T + 1, 0);
    w.size.assign((size_t)T + 1, 1);
    if (n_planes > 1)   // :71  one slice: the plane labelling is the answer
        for (int pass = 0; pass < 2; ++pass)
            if (!w.pass(pass == 1)) {
                sk::set_error("sk_stitch_walk_host: the stitched ids pass INT32_MAX");
                return SK_ERR_CAPACITY;
            }
    int32_t mx = 0;
    lut_host[0] = 0;
    for (int c = 1; c <= T; ++c) {
        lut_host[c] = w.cur[c];
        mx = std::max(mx, w.cur[c]);
    }
    *max_label_host = mx;
    return SK_OK;
}
