// Stand-alone run of the coefficient-table derivation (rr_plan.hpp: tributary_weight, lag_coef, reach_coef, tile_coef and its masked forms), compiled with
// river_route_amd/csrc/rr_plan.cpp by tests/test_coef_tables.py -- plainly and under the address / undefined-behaviour sanitizers.
// Reads the case file named on the command line (whitespace-separated; integers in decimal, doubles as 16-digit hex words):
//   n n_edges block lanes wmax | indptr[n + 1] | indices[n_edges] | n_ghost ghost reaches | n_sets | per set: has_lhs has_c4,
//   lhs_off_data[n_edges] if has_lhs, c2[n], c3[n], c4_dt[n] if has_c4
// and prints one line per table, "<name> <64-bit hex words>": `info`, then per set s `s.differ`, `s.reach`, the lag-order arrays, the
// tile-order table with the ghost list (`s.tile`), the in-pass eligibility mask the engine would take from it and the three masked
// forms, the skeleton's table where the direct row path applies; `s.member_c1row`; last `members`: the sets as rr_plan_set_member_coeffs stages them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../river_route_amd/csrc/rr_plan.hpp"

namespace {
std::ifstream in;
int64_t integer() { std::string t; in >> t; return std::stoll(t); }
double word() { std::string t; in >> t; const uint64_t u = std::stoull(t, nullptr, 16); double x; std::memcpy(&x, &u, sizeof x); return x; }
std::vector<double> words(int64_t count) { std::vector<double> v((size_t)count); for (double &x : v) x = word(); return v; }

void line(const std::string &name, const std::vector<double> &v)
{
    std::printf("%s", name.c_str());
    for (double x : v) { uint64_t u; std::memcpy(&u, &x, sizeof u); std::printf(" %016llx", (unsigned long long)u); }
    std::printf("\n");
}
void line(const std::string &name, const std::vector<int64_t> &v)
{
    std::printf("%s", name.c_str());
    for (int64_t x : v) std::printf(" %016llx", (unsigned long long)x);
    std::printf("\n");
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    in.open(argv[1]);
    if (!in) return 2;
    const int64_t n = integer(), n_edges = integer();
    const int32_t block = (int32_t)integer(), lanes = (int32_t)integer(), wmax = (int32_t)integer();
    std::vector<int32_t> indptr((size_t)n + 1), indices((size_t)n_edges);
    for (int32_t &v : indptr) v = (int32_t)integer();
    for (int32_t &v : indices) v = (int32_t)integer();
    std::vector<int32_t> ghosts((size_t)integer());
    for (int32_t &v : ghosts) v = (int32_t)integer();

    rr::HostPlan H;
    std::string err;
    if (rr::build_host_plan(n, indptr.data(), indices.data(), H, err)) { std::printf("plan failed: %s\n", err.c_str()); return 1; }
    std::vector<int32_t> lag_of((size_t)n);
    for (int64_t i = 0; i < n; ++i) lag_of[i] = H.lag[H.inv[i]];
    rr::TilePlan T;
    rr::build_tile_plan(H.down, lag_of, block, T);
    rr::DirectPlan D;
    rr::build_direct_plan(H.down, lag_of, lanes, wmax, block, D);
    if (!T.ok) { std::printf("the network does not tile\n"); return 1; }
    line("info", std::vector<int64_t>{T.np, T.n_ghost, T.n_tiles, T.n_levels, D.ok ? 1 : 0, D.skel.np, D.n_holes});

    const int32_t boundary = 1 << 30;
    std::vector<int32_t> lag(T.lag);      // with the boundary ghosts' flag, as the engine hands it to mark_inpass_headwaters
    for (int32_t i : ghosts) lag[T.inv[i]] |= boundary;

    const int64_t n_sets = integer();
    std::vector<double> staged((size_t)(n_sets * 3 * T.np), -777.0), reach(4 * (size_t)n);      // (the engine's staging starts unfilled: every position must be written)
    for (int64_t s = 0; s < n_sets; ++s) {
        const bool has_lhs = integer() != 0, has_c4 = integer() != 0;
        const std::vector<double> lhs = words(has_lhs ? n_edges : 0), c2 = words(n), c3 = words(n), c4 = words(has_c4 ? n : 0);
        const std::string k = std::to_string(s) + ".";
        const double *lhs_or_null = has_lhs ? lhs.data() : nullptr;
        rr::LagCoef L;
        std::vector<double> c1row_own((size_t)n);
        const int64_t differ = rr::lag_coef(H, lhs_or_null, c2.data(), c3.data(), has_c4 ? c4.data() : nullptr, L, c1row_own.data());
        rr::reach_coef(n, c1row_own.data(), c2.data(), c3.data(), has_c4 ? c4.data() : nullptr, reach.data());
        line(k + "differ", std::vector<int64_t>{differ});
        line(k + "reach", reach);
        line(k + "w", L.w); line(k + "c1row", L.c1row); line(k + "c2", L.c2); line(k + "c3", L.c3); line(k + "c4", L.c4);

        std::vector<double> tile(3 * (size_t)T.np), plain(tile), dense(tile);
        rr::tile_coef(T, rr::table_rows(reach.data()), rr::kTileGhost, ghosts, tile.data());      // as rr_plan_set_boundary lays it out
        line(k + "tile", tile);
        rr::tile_coef(T, rr::ReachCoef{c1row_own.data(), c2.data(), c3.data(), 1}, rr::kTileGhost, ghosts, dense.data());      // as rr_plan_set_coeffs does
        line(k + "tile_dense", dense);
        rr::tile_coef(T, rr::table_rows(reach.data()), rr::kTileGhost, {}, plain.data());      // the same before the ghost list is known
        line(k + "tile_no_list", plain);
        std::vector<uint8_t> elig;
        rr::mark_inpass_headwaters(T, lag, boundary, elig, nullptr, tile.data());
        line(k + "elig", std::vector<int64_t>(elig.begin(), elig.end()));
        std::vector<double> masked(tile), col(3 * (size_t)n);
        rr::zero_tile_coef(masked.data(), elig);
        line(k + "tile_hw", masked);
        masked = tile;
        rr::zero_tile_coef_headwaters(T, masked.data());
        line(k + "tile_unit", masked);
        rr::column_coef(T, tile.data(), n, col.data());
        line(k + "col", col);
        if (D.ok) {
            std::vector<double> skel(3 * (size_t)D.skel.np);
            rr::tile_coef(D.skel, rr::table_rows(reach.data()), rr::kTileGhost, {}, skel.data());
            line(k + "skel", skel);
        }
        std::vector<double> c1row((size_t)n), w;      // member s's slice, from its own arrays beside its c1row: no per-reach table
        if (rr::tributary_weight(H, lhs_or_null, w, c1row.data()) != differ || w != L.w) return 3;
        line(k + "member_c1row", c1row);
        rr::tile_coef(T, rr::ReachCoef{c1row.data(), c2.data(), c3.data(), 1}, rr::kTileGhost, ghosts, staged.data() + s * 3 * T.np);
    }
    line("members", staged);
    return 0;
}
