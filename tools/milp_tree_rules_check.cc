// milp_tree_rules_check.cc -- the search rules of yalps_amd/csrc/milp_tree_rules.cuh under the host's sanitizers.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__host__= -D__device__= \
//       -o /tmp/milp_tree_rules_check tools/milp_tree_rules_check.cc && /tmp/milp_tree_rules_check
// Drives a few thousand random trees with a synthetic evaluator -- status, result and column 0 a fixed hash of the cut list,
// many equal results -- through mt_begin / mt_next / mt_consume on arenas of 2 entries and up, each arena allocated at its
// exact size (so that a write past it is a heap overflow the sanitizer reports), rerun at x 4 after MT_ARENA_FULL as the
// library does, and checks that a rerun repeats the tree's pop sequence as far as the smaller arena got.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yalps_amd/csrc/milp_tree_rules.cuh"

static uint64_t mix(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

static uint64_t hash_cuts(uint64_t seed, const MtArena &a, int32_t slot) {
    uint64_t h = mix(seed);
    for (int32_t q = 0; q < a.slot_n[slot]; q++) {
        const size_t at = (size_t)slot * a.maxcuts + q;
        uint64_t bits;
        std::memcpy(&bits, &a.cut_val[at], sizeof bits);
        h = mix(h ^ (uint64_t)(uint32_t)a.cut_sv[2 * at] ^ ((uint64_t)(uint32_t)a.cut_sv[2 * at + 1] << 32));
        h = mix(h ^ bits);
    }
    return h;
}

int main() {
    static const double results[] = {-0.0, 0.0, 1.0, 1.0, 1.5, 2.0, 2.0, 3.0, -1.0, NAN, INFINITY};
    static const double values[] = {0.0, 1.0, 2.0, 0.5, 1.5, 2.5, 0.25, 3.75, -0.5, -0.0, NAN};
    long trees = 0, nodes = 0, reruns = 0, overflows = 0;
    for (uint64_t seed = 1; seed <= 3000; seed++) {
        const int32_t nints = 1 + (int32_t)(mix(seed) % 12), w = nints + 3, h0 = nints + 2, maxcuts = 2 * nints;
        std::vector<int32_t> ints(nints), pos((size_t)w + h0 + maxcuts);
        for (int32_t k = 0; k < nints; k++) ints[k] = k + 1;
        std::vector<double> col0((size_t)h0 + maxcuts);
        const double max_iter[] = {0.0, 1.0, 2.5, 60.0, 400.0, NAN, INFINITY};
        const double tol[] = {0.0, 0.0, 0.5, NAN, INFINITY};
        const MtTree T = {w, nints, ints.data(), (seed & 1) ? 1.0 : -1.0, 1e-8, tol[mix(seed ^ 7) % 5], max_iter[mix(seed ^ 5) % 7],
                          (int32_t)(mix(seed ^ 9) % 17 == 0)};
        const uint64_t frac_pct = 30 + mix(seed ^ 11) % 35; // subcritical to slightly supercritical trees
        std::vector<uint64_t> first_seq;
        const int32_t caps[] = {2, 3, 5, 8, 16};
        for (int32_t cap = caps[seed % 5];; cap *= 4) {
            if (cap > 4096) {
                overflows++;
                break;
            }
            std::vector<double> mem(mt_arena_doubles(cap, maxcuts)); // (exactly the arena: one entry past it is the sanitizer's)
            const MtArena A = mt_arena_bind(mem.data(), cap, maxcuts);
            auto view = [&](uint64_t h, int32_t rows, bool integral) {
                for (int32_t j = 0; j < rows; j++) {
                    const double v = values[mix(h ^ (uint64_t)j) % 11];
                    col0[j] = integral ? (v == v ? floor(v) : 0.0) : v;
                }
                for (int32_t p = 0; p < w + rows; p++) pos[p] = p;
                for (int32_t k = 0; k < nints; k++)
                    if (mix(h ^ (0x100u + k)) % 5 != 0) pos[ints[k]] = w + k + 1; // basic in row k + 1
            };
            view(mix(seed ^ 13), h0, false);
            mt_begin(T, A, (int32_t)(mix(seed ^ 15) % 11 == 0), results[mix(seed ^ 17) % 11], col0.data(), pos.data());
            std::vector<uint64_t> seq;
            long guard = 0;
            while (mt_next(T, A) && guard++ < 20000) {
                const int32_t slot = A.state->cur_slot, h = h0 + A.slot_n[slot];
                const uint64_t key = hash_cuts(seed, A, slot);
                seq.push_back(key);
                const uint64_t u = mix(key ^ 1) % 100;
                int32_t st = 1;
                double res = NAN;
                if (u < frac_pct + 20) {
                    st = 0, res = results[mix(key ^ 2) % 11];
                    view(key, h, u >= frac_pct);
                } else if (u < frac_pct + 30) {
                    st = 3;
                }
                nodes++;
                if (mt_consume(T, A, st, res, col0.data(), pos.data(), h) == MT_ARENA_FULL) break;
            }
            if (guard >= 20000) A.state->status = MT_TIMEDOUT; // (a supercritical tree under maxIterations = inf: cut short here)
            const size_t common = first_seq.size() < seq.size() ? first_seq.size() : seq.size();
            if (!first_seq.empty() && std::memcmp(first_seq.data(), seq.data(), common * sizeof(uint64_t)) != 0) {
                std::fprintf(stderr, "seed %llu: the rerun at %d entries pops another sequence\n", (unsigned long long)seed, cap);
                return 1;
            }
            if (seq.size() < first_seq.size()) {
                std::fprintf(stderr, "seed %llu: the rerun at %d entries ended before the smaller arena did\n", (unsigned long long)seed, cap);
                return 1;
            }
            first_seq.swap(seq);
            if (A.state->heap_n > cap || A.state->free_n < 0 || A.state->free_n > cap + 1) {
                std::fprintf(stderr, "seed %llu: heap_n %d free_n %d outside an arena of %d\n", (unsigned long long)seed, A.state->heap_n,
                             A.state->free_n, cap);
                return 1;
            }
            if (A.state->status != MT_ARENA_FULL) break;
            reruns++;
        }
        trees++;
    }
    std::printf("milp_tree_rules_check: %ld trees, %ld nodes, %ld reruns, %ld above 4096 entries: ok\n", trees, nodes, reruns, overflows);
    return 0;
}
