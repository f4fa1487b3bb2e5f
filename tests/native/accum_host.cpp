// accum_host.cpp — TEST ONLY: the accumulator's passes (rt_mega.h, chain buffer) on the host:
// mega_emu.h's emulation of rt_mega_kernel in its CHAIN form, over the records in `chain`.
// Built together with kernel_host.cpp, whose default options (and setters) the passes use.
#include "mega_emu.h"

extern emu::Options kh_options;   // kernel_host.cpp

// Fresh records of the shard's n pixels (rt_chain_init_kernel).
extern "C" void kh_accum_init(const rt_scene_view *v, int rank, int world, int row_block, uint32_t *chain) {
    const rtd::DevScene sc = emu::make(v);
    const emu::Shard sh = emu::shard_of(v, rank, world, row_block);
    for (long long p = 0; p < sh.n; ++p) rtd::chain_init((uint4 *)chain, sc, sh.g, (int)p);
}

// One pass to absolute sample s1 over the records in `chain` (8 words per shard pixel).
// mode 0: the plain emulation; 1: the runahead emulation; 2: the hand-off (the plain emulation
// parks its sparse tail waves below park_below held pixels, the runahead emulation resumes).
extern "C" int kh_accum_pass(const rt_scene_view *v, int s1, int rank, int world, int row_block, int waves,
                             int shade_min, int mode, int park_below, uint32_t *chain, float *out,
                             uint64_t *parked_out) {
    emu::Options &o = kh_options;
    o.chain = (uint4 *)chain;
    int rc;
    if (mode == 0) rc = emu::render_mega<false, false, true>(v, s1, rank, world, row_block, waves, shade_min, nullptr, out, nullptr, o);
    else if (mode == 1) rc = emu::render_mega<false, true, true>(v, s1, rank, world, row_block, waves, shade_min, nullptr, out, nullptr, o);
    else rc = emu::render_mega_handoff<true>(v, s1, rank, world, row_block, waves, waves, shade_min, park_below, 100, nullptr,
                                            out, nullptr, parked_out, o);
    o.chain = nullptr;
    return rc;
}
