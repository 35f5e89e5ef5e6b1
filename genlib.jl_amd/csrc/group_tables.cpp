// group_tables.cpp -- build_group_tables (group_tables.h).  No HIP here.
#include "group_tables.h"

#include <algorithm>
#include <climits>

namespace genphi {

void build_group_tables(const int32_t *group, int n_groups, int64_t N, int64_t row_begin, int64_t n_rows, int n_cus, GroupTables &t)
{
    const int G = n_groups;
    const int64_t r0 = row_begin, nr = n_rows;
    t = GroupTables();
    // labels: counts, and whether every group's columns are one run (form 0)
    t.n_cols.assign(G, 0);
    t.n_rows.assign(G, 0);
    int form = 0;
    {
        std::vector<char> closed(G, 0);
        for (int64_t i = 0; i < N; ++i) {
            const int g = group[i];
            if (i > 0 && group[i - 1] >= 0 && group[i - 1] != g) closed[group[i - 1]] = 1;
            if (g < 0) continue;
            if (closed[g]) form = 1;
            ++t.n_cols[g];
            if (i >= r0 && i < r0 + nr) ++t.n_rows[g];
        }
    }
    t.form = form;
    // resident rows sorted by group (stable), cut into blocks of one group and at most kGsBlockRows rows of even size
    std::vector<int> &rowlist = t.rowlist;
    std::vector<GsPair> &blocks = t.blocks;
    std::vector<int> cnt(G, 0);                       // rows of `part` per group
    {
        std::vector<int64_t> at(G + 1, 0);
        for (int g = 0; g < G; ++g) at[g + 1] = at[g] + t.n_rows[g];
        rowlist.resize(static_cast<size_t>(at[G]));
        std::vector<int64_t> fill(at.begin(), at.end() - 1);
        for (int64_t k = 0; k < nr; ++k)
            if (group[r0 + k] >= 0) rowlist[static_cast<size_t>(fill[group[r0 + k]]++)] = static_cast<int>(k);
        for (int g = 0; g < G; ++g) {
            const int64_t n = t.n_rows[g], nb = (n + kGsBlockRows - 1) / kGsBlockRows;
            int64_t first = at[g];
            for (int64_t b = 0; b < nb; ++b) {
                const int64_t len = n / nb + (b < n % nb ? 1 : 0);
                blocks.push_back(GsPair{static_cast<int>(first), static_cast<int>(len)});
                first += len;
            }
            cnt[g] = static_cast<int>(nb);
        }
    }
    const int64_t n_blocks = static_cast<int64_t>(blocks.size());
    if (n_blocks == 0) return;

    // column tiles: pieces (list A) and the pieces of each group (list B), the same for every row
    const int n_tiles = t.n_tiles = static_cast<int>((N + kGsTile - 1) / kGsTile);
    std::vector<GsPair> &tile_lists = t.tile_lists;
    std::vector<int> &list_a = t.list_a;
    std::vector<GsPair> &list_b = t.list_b;
    std::vector<unsigned short> &perm = t.perm;
    tile_lists.resize(static_cast<size_t>(n_tiles) + 1);
    perm.assign(form ? static_cast<size_t>(n_tiles) * kGsTile : 0, 0);
    {
        std::vector<unsigned short> seq;              // form 0: the tile's labelled columns; form 1: those sorted by group = perm
        for (int tl = 0; tl < n_tiles; ++tl) {
            tile_lists[tl] = GsPair{static_cast<int>(list_a.size()), static_cast<int>(list_b.size())};
            const int64_t c0 = static_cast<int64_t>(tl) * kGsTile;
            const int tw = static_cast<int>(std::min<int64_t>(kGsTile, N - c0));
            seq.clear();
            for (int c = 0; c < tw; ++c) if (group[c0 + c] >= 0) seq.push_back(static_cast<unsigned short>(c));
            if (form) {
                std::stable_sort(seq.begin(), seq.end(), [&](unsigned short x, unsigned short y) { return group[c0 + x] < group[c0 + y]; });
                std::copy(seq.begin(), seq.end(), perm.begin() + static_cast<size_t>(tl) * kGsTile);
            }
            const int a0 = static_cast<int>(list_a.size());
            for (size_t s = 0; s < seq.size();) {       // one group: its pieces, then its entry of list B
                const int g = group[c0 + seq[s]];
                const int first_piece = static_cast<int>(list_a.size()) - a0;
                size_t e = s;
                while (e < seq.size() && group[c0 + seq[e]] == g && (form || e == s || seq[e] == seq[e - 1] + 1)) ++e;
                for (size_t q = s; q < e; q += kGsPiece)
                    list_a.push_back((form ? static_cast<int>(q) : static_cast<int>(seq[q])) | static_cast<int>(std::min<size_t>(kGsPiece, e - q)) << 16);
                list_b.push_back(GsPair{first_piece | (static_cast<int>(list_a.size()) - a0 - first_piece) << 16, g});
                s = e;
            }
        }
        tile_lists[n_tiles] = GsPair{static_cast<int>(list_a.size()), static_cast<int>(list_b.size())};
    }
    // enough workgroups to fill the device several times over: column slabs
    const int64_t want_wgs = 24LL * std::max(n_cus, 1);
    const int slabs_want = static_cast<int>(std::min<int64_t>(n_tiles, std::max<int64_t>(1, (want_wgs + n_blocks - 1) / n_blocks)));
    t.tiles_per_slab = (n_tiles + slabs_want - 1) / slabs_want;
    const int n_slabs = t.n_slabs = (n_tiles + t.tiles_per_slab - 1) / t.tiles_per_slab;
    t.n_part = n_blocks * n_slabs;
    if (t.n_part > INT32_MAX / 2) return;
    // levels of the row reduction: at most kGsFan rows of one group per output row; the last level has one row per group
    for (int g = 0; g < G; ++g) cnt[g] *= n_slabs;
    for (;;) {
        const bool last = *std::max_element(cnt.begin(), cnt.end()) <= kGsFan;
        std::vector<int> beg(1, 0);
        int at = 0;
        for (int g = 0; g < G; ++g) {
            const int n = cnt[g], outs = last ? 1 : (n + kGsFan - 1) / kGsFan;
            for (int o = 0; o < outs; ++o) {
                at += last ? n : std::min(kGsFan, n - o * kGsFan);
                beg.push_back(at);
            }
            cnt[g] = outs;
        }
        t.level_rows.push_back(static_cast<int64_t>(beg.size()) - 1);
        t.level_beg.push_back(std::move(beg));
        if (last) break;
    }
}

}  // namespace genphi
