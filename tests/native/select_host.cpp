// select_host.cpp — TEST ONLY: rt_select.h (the subset passes' selection rule) and the subset
// fields of rt_launch_plan.h behind a C interface for tests/test_select.py.  Both headers are
// host-compilable, so this builds with plain g++ (with -ffp-contract=off, as every unit that
// includes rt_select.h).  sh_select restates rt_select_kernel's contract on the host: one rule
// evaluation per shard pixel, the list in ascending shard-pixel order, and the reductions.
//
// Built a second time with -DSELECT_HOST_MAIN it is a stand-alone program (for the sanitizer
// run): `select_host in.bin out.bin` reads cases, runs sh_select on each and writes the lists.
//   in.bin   i32 n_cases, then per case: 12 x i32 (width, height, rank, world, row_block, target,
//            x0, y0, x1, y1, has_mask, n_pixels), f32 threshold, i32 n_b[n], f32 S_b[3n],
//            i32 n_a[n], f32 S_a[3n], u8 mask[n] (present if has_mask)
//   out.bin  per case: i64 n_selected, u64 samples, i32 next_min, next_max, i32 list[n_selected]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raytracing-hw_amd/csrc/rt_select.h"
#include "plan_io.h"

extern "C" {

struct sh_rule {
    int target, x0, y0, x1, y1;
    float threshold;
};

static rtsel::Rule rule_of(const sh_rule *r) { return rtsel::Rule{r->target, r->x0, r->y0, r->x1, r->y1, r->threshold}; }

int sh_check_rule(const sh_rule *r, int width, int height) { return rtsel::check_rule(rule_of(r), width, height); }
float sh_count_normalizer(int n) { return rtsel::count_normalizer(n); }
float sh_error_estimate(int n_a, const float *S_a, int n_b, const float *S_b) { return rtsel::error_estimate(n_a, S_a, n_b, S_b); }

// The shard (rank of world, blocks of row_block rows) of a width x height frame: shard pixel p is
// (p % width, the (p / width)-th owned row).  n_b, S_b, n_a, S_a, mask (may be NULL): per shard
// pixel.  list: room for every shard pixel.  e_out (may be NULL): step 4's estimate where the
// rule reaches it, NaN elsewhere.  Returns the list's length, or -1 when n_pixels does not fit.
long long sh_select(const sh_rule *r, int width, int height, int rank, int world, int row_block, long long n_pixels,
                    const int *n_b, const float *S_b, const int *n_a, const float *S_a, const uint8_t *mask, int *list,
                    float *e_out, unsigned long long *samples, int *next_min, int *next_max) {
    const rtsel::Rule rule = rule_of(r);
    std::vector<int> rows;
    for (int y = 0; y < height; ++y)
        if ((y / row_block) % world == rank) rows.push_back(y);
    if ((long long)rows.size() * width != n_pixels) return -1;
    long long n = 0;
    unsigned long long s = 0;
    int lo = std::numeric_limits<int>::max(), hi = 0;
    for (long long p = 0; p < n_pixels; ++p) {
        const int x = (int)(p % width), y = rows[(size_t)(p / width)];
        const bool sel = rtsel::selected(rule, x, y, mask ? mask[p] : 1u, n_b[p], S_b + 3 * p, n_a[p], S_a + 3 * p);
        if (e_out)
            e_out[p] = n_a[p] > 0 && n_b[p] > n_a[p] ? rtsel::error_estimate(n_a[p], S_a + 3 * p, n_b[p], S_b + 3 * p)
                                                    : std::numeric_limits<float>::quiet_NaN();
        const int after = sel ? rule.target : n_b[p];
        lo = after < lo ? after : lo;
        hi = after > hi ? after : hi;
        if (sel) {
            list[n++] = (int)p;
            s += (unsigned long long)(rule.target - n_b[p]);
        }
    }
    if (samples) *samples = s;
    if (next_min) *next_min = lo;
    if (next_max) *next_max = hi;
    return n;
}

// The launch plan (plan_io.h), for the subset fields.
int sh_plan(const plan_in *i, plan_out *o) { return plan_fill(i, o); }

}  // extern "C"

#ifdef SELECT_HOST_MAIN
namespace {
template <class T>
bool get(std::FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: select_host in.bin out.bin\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "select_host: cannot open files\n");
        return 2;
    }
    int32_t n_cases = 0;
    if (std::fread(&n_cases, 4, 1, in) != 1) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t h[12];
        float thr;
        if (std::fread(h, 4, 12, in) != 12 || std::fread(&thr, 4, 1, in) != 1 || h[11] < 0) return 3;
        const size_t n = (size_t)h[11];
        std::vector<int32_t> n_b, n_a, list(n ? n : 1);
        std::vector<float> S_b, S_a;
        std::vector<uint8_t> mask;
        if (!get(in, n_b, n) || !get(in, S_b, 3 * n) || !get(in, n_a, n) || !get(in, S_a, 3 * n)) return 3;
        if (h[10] && !get(in, mask, n)) return 3;
        const sh_rule r{h[5], h[6], h[7], h[8], h[9], thr};
        unsigned long long samples = 0;
        int32_t lo = 0, hi = 0;
        const long long k = sh_select(&r, h[0], h[1], h[2], h[3], h[4], (long long)n, n_b.data(), S_b.data(), n_a.data(),
                                      S_a.data(), h[10] ? mask.data() : nullptr, list.data(), nullptr, &samples, &lo, &hi);
        if (k < 0) return 4;
        const int64_t k64 = k;
        std::fwrite(&k64, 8, 1, out);
        std::fwrite(&samples, 8, 1, out);
        std::fwrite(&lo, 4, 1, out);
        std::fwrite(&hi, 4, 1, out);
        if (k) std::fwrite(list.data(), 4, (size_t)k, out);
        // the plan's subset rule on this case's numbers, for the sanitizers' benefit
        plan_in pi{0, 0, 0, 0, r.target, 1, (long long)n, 8, 100, 1024, 1024, k, 0, 0, 0};
        plan_out po;
        if (k > 0 && n > 0 && (sh_plan(&pi, &po) != 0 || po.n_items != k || po.ordered)) return 5;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 6;
}
#endif
