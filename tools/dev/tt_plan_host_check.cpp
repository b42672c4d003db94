// Stand-alone check of the two-team kernel's work-item plan (csrc/conv_tt.hpp tt_plan_items: which tiles exist, which XCD queue gets
// them), meant for a sanitizer build on a machine without a GPU (tools/dev/README.md).  Every shape is the smallest at which the index
// arithmetic can go wrong.  Per case: every (member, channel block, tile) occurs exactly once, the tiles cover the stacked rows and the
// columns, `first` is monotone and ends at the item count, a member's slices are contiguous in tile-major order, the members of a queue
// follow each other by `chunks` descending, `lazy` follows items < 3 * n_wgs, and the FNV-1a hash over the item bytes and `first` equals a
// constant RECORDED FROM THE LOOP THIS FILE'S COMMIT MOVED (tt_build_plan in hrnet.cpp, run on the same inputs): the move into the
// kernel's header changed no byte.  The cases added later for widths no packaged config has (partial last 64-channel blocks behind full
// ones, 3 and 5 blocks of 96) are STRUCTURAL: they carry no recorded hash (NO_HASH), only the coverage checks.  Nothing here touches a device.
#include "../../soccernet-calibration-sportlight_amd/csrc/conv_tt.hpp"
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

using namespace sncal;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d (%s): %s\n", __FILE__, __LINE__, case_name, #c); ++fails; } } while (0)

static TTMember member(int N, int H, int W, int cout, int chunks) {
    TTMember m;
    memset(&m, 0, sizeof m);
    m.N = N; m.H = H; m.W = W; m.cout = cout; m.chunks = chunks;
    return m;
}

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

constexpr uint64_t NO_HASH = 0;          // a structural case: no hash was recorded for it

static void check_plan(const char* case_name, const TTMember* mem, int n, TTTile tile, int n_wgs, uint64_t want = NO_HASH) {
    const TTPlan plan = tt_plan_items(mem, n, tile, n_wgs);
    const TTTileInfo& t = TT_TILES[tile];
    long total = 0;
    for (int m = 0; m < n; ++m) total += tt_grid(mem[m].N, mem[m].H, mem[m].W, mem[m].cout, tile).items();
    const size_t count = plan.first[8];
    CHECK((long)count == total);
    CHECK(plan.items.size() == (count ? count : 1));                   // nothing to do: the one dummy item
    if (!count) CHECK(plan.items[0].member == 0 && plan.items[0].nb == 0 && plan.items[0].row0 == 0 && plan.items[0].col0 == 0 && plan.items[0].pad_ == 0);
    CHECK(plan.first[0] == 0);
    for (int x = 0; x < 8; ++x) {
        CHECK(plan.first[x] <= plan.first[x + 1]);
        if (n_wgs < 8 && x > 0) CHECK(plan.first[x] == count);        // a single queue
    }
    CHECK(plan.lazy == (plan.items.size() < (size_t)3 * (size_t)n_wgs ? 1 : 0));
    std::set<std::tuple<int, int, int, int>> seen;
    long next[TT_MAX_MEMBERS] = {0, 0, 0};                            // per member: the tile-major index its next item must have
    int rows_end[TT_MAX_MEMBERS] = {0, 0, 0}, cols_end[TT_MAX_MEMBERS] = {0, 0, 0};
    std::set<int> blocks_seen[TT_MAX_MEMBERS];
    for (int x = 0; x < 8 && plan.first[x] <= plan.first[x + 1] && plan.first[x + 1] <= plan.items.size(); ++x) {
        int prev_chunks = 1 << 30, prev_member = -1, runs = 0;
        for (uint32_t i = plan.first[x]; i < plan.first[x + 1]; ++i) {
            const TTItem& it = plan.items[i];
            CHECK(it.member < n && it.pad_ == 0);
            if (it.member >= n) continue;
            const TTMember& m = mem[it.member];
            const TTGrid g = tt_grid(m.N, m.H, m.W, m.cout, tile);
            CHECK(it.nb < g.nblk && it.row0 >= 0 && it.col0 >= 0 && it.row0 % t.tile_h == 0 && it.col0 % t.tile_w == 0);
            CHECK(it.row0 < m.N * (m.H + 1) && it.col0 < m.W && (int)it.nb * t.cout_blk < m.cout);
            CHECK(seen.insert(std::make_tuple((int)it.member, (int)it.nb, (int)it.row0, (int)it.col0)).second);
            blocks_seen[it.member].insert((int)it.nb);
            rows_end[it.member] = std::max(rows_end[it.member], it.row0 + t.tile_h);
            cols_end[it.member] = std::max(cols_end[it.member], it.col0 + t.tile_w);
            // slice x of a member continues where slice x - 1 ended, tile-major with the channel blocks of a tile adjacent
            const long idx = ((long)(it.row0 / t.tile_h) * g.tiles_x + it.col0 / t.tile_w) * g.nblk + it.nb;
            CHECK(idx == next[it.member]);
            next[it.member] = idx + 1;
            if (it.member != prev_member) { ++runs; CHECK(m.chunks < prev_chunks); prev_chunks = m.chunks; prev_member = it.member; }
        }
        CHECK(runs <= n);                                              // one run per member and queue
    }
    CHECK(seen.size() == count);
    for (int m = 0; m < n; ++m) {
        const TTGrid g = tt_grid(mem[m].N, mem[m].H, mem[m].W, mem[m].cout, tile);
        CHECK(next[m] == g.items());
        // the channel blocks [0, ceil(cout / blk)) all occur, the last one holds at least one real channel and no block lies beyond the width
        CHECK((int)blocks_seen[m].size() == g.nblk && g.nblk == (mem[m].cout + t.cout_blk - 1) / t.cout_blk);
        CHECK((g.nblk - 1) * t.cout_blk < mem[m].cout && g.nblk * t.cout_blk >= mem[m].cout);
        CHECK(rows_end[m] >= mem[m].N * (mem[m].H + 1) && rows_end[m] - t.tile_h < mem[m].N * (mem[m].H + 1));      // rows [0, N (H + 1)) covered, no tile beyond
        CHECK(cols_end[m] >= mem[m].W && cols_end[m] - t.tile_w < mem[m].W);
    }
    uint64_t h = fnv(1469598103934665603ull, plan.items.data(), plan.items.size() * sizeof(TTItem));
    h = fnv(h, plan.first, sizeof plan.first);
    h = fnv(h, &plan.lazy, sizeof plan.lazy);
    if (want != NO_HASH && h != want) { printf("FAILED %-34s %016llx, recorded %016llx\n", case_name, (unsigned long long)h, (unsigned long long)want); ++fails; }
}

int main() {
    const char* case_name = "shapes";
    static_assert(sizeof(TTItem) == 16, "the hashes cover the items as the kernel reads them");
    CHECK(TT_TILES[TT_TILE_96x8].cout_blk == 96 && TT_TILES[TT_TILE_96x8].tile_h == 8 && TT_TILES[TT_TILE_64x12].cout_blk == 64 &&
          TT_TILES[TT_TILE_64x12].tile_h == 12 && TT_TILES[TT_TILE_96x4].cout_blk == 96 && TT_TILES[TT_TILE_96x4].tile_h == 4);
    const TTMember one = member(1, 1, 1, 96, 3);
    // three members of different cost, given out of order: 3 x (17 + 1) = 54 stacked rows (a partial last tile of 8 and of 4 rows), 30 columns
    // (a partial column tile), 1 / 2 / 4 channel blocks
    const TTMember three[3] = {member(3, 17, 30, 192, 6), member(3, 17, 30, 384, 12), member(3, 17, 30, 96, 3)};
    const TTMember narrow = member(3, 17, 30, 48, 3);                 // one padded 64-channel block
    const TTMember wide = member(1, 17, 33, 96, 3);                   // two column tiles, the second one pixel wide
    check_plan("1x1x1 cout 96, 96x8", &one, 1, TT_TILE_96x8, 256, 0xbcc7c093a8ac0152ull);
    check_plan("3 members 3x17x30, 96x8", three, 3, TT_TILE_96x8, 256, 0x476e9682aedafa3cull);
    check_plan("3 members 3x17x30, 96x4", three, 3, TT_TILE_96x4, 256, 0x1c7d2b65b05b8034ull);
    check_plan("3 members 3x17x30, 96x8, 4 wgs", three, 3, TT_TILE_96x8, 4, 0xfb2f5223ca4b9020ull);
    check_plan("cout 48 3x17x30, 64x12", &narrow, 1, TT_TILE_64x12, 256, 0x9eec499e4445d5f0ull);
    check_plan("1x17x33 cout 96, 96x8", &wide, 1, TT_TILE_96x8, 256, 0x971ad065266ff4b0ull);
    check_plan("1x17x33 cout 96, 96x8, 4 wgs", &wide, 1, TT_TILE_96x8, 4, 0x9de2b19eba7d1db2ull);
    check_plan("no member", three, 0, TT_TILE_96x8, 256, 0xa81fa6c2b00d6792ull);
    // ---- structural cases: widths beyond the packaged configs (tests/width_cases.py), 3 frames of the 9x13 / 5x7 / 3x4 maps ----
    // 64 x 12 tile (split engine, launched alone): 176 = 2 full blocks + 48 channels, 400 = 6 full blocks + 16; 3 x (9 + 1) = 30 stacked
    // rows are 2 1/2 tiles of 12, 3 x (3 + 1) = 12 rows exactly one
    const TTMember c176 = member(3, 9, 13, 176, 11), c400 = member(3, 3, 4, 400, 25);
    check_plan("cout 176 3x9x13, 64x12", &c176, 1, TT_TILE_64x12, 256);
    check_plan("cout 400 3x3x4, 64x12", &c400, 1, TT_TILE_64x12, 256);
    check_plan("cout 400 3x3x4, 64x12, 4 wgs", &c400, 1, TT_TILE_64x12, 4);
    // 96-channel tiles: 3 blocks (288) and the admitted maximum of 5 (480), on the 8-row and the 4-row tile
    const TTMember c288 = member(3, 9, 13, 288, 9), c480 = member(3, 5, 7, 480, 15);
    for (TTTile tile : {TT_TILE_96x8, TT_TILE_96x4}) {
        check_plan(tile == TT_TILE_96x8 ? "cout 288 3x9x13, 96x8" : "cout 288 3x9x13, 96x4", &c288, 1, tile, 256);
        check_plan(tile == TT_TILE_96x8 ? "cout 480 3x5x7, 96x8" : "cout 480 3x5x7, 96x4", &c480, 1, tile, 256);
    }
    // launches that share: stage 2's pair 96 + 288 = 384 channels (maps 18x26 and 9x13), given cheap member first; three members
    // 96 + 288 + 288 = 672 <= TT_COUT_MAX of different cost
    const TTMember pair[2] = {member(3, 18, 26, 96, 3), member(3, 9, 13, 288, 9)};
    const TTMember trio[3] = {member(3, 18, 26, 96, 3), member(3, 9, 13, 288, 9), member(3, 5, 7, 288, 18)};
    for (TTTile tile : {TT_TILE_96x8, TT_TILE_96x4}) {
        check_plan(tile == TT_TILE_96x8 ? "pair 96 + 288, 96x8" : "pair 96 + 288, 96x4", pair, 2, tile, 256);
        check_plan(tile == TT_TILE_96x8 ? "trio 96 + 288 + 288, 96x8" : "trio 96 + 288 + 288, 96x4", trio, 3, tile, 256);
    }
    printf(fails ? "tt_plan_host_check: %d FAILED\n" : "tt_plan_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
