// rt_records.h — an accumulator's 32-byte per-pixel records (host and device, no HIP).
//
// The one text of their layout.  The records are a device format (the chain buffer and the
// moment buffer of rt_accum_device.h, the park list of rt_mega.h) and a file format
// (rt_accum_file.h) at once: 8 little-endian 32-bit words each, floats by their bits.
//   parity  (rt_accum_create, and a parked pixel of the hand-off): pixel, next sample, engine
//           state with the normal-cache flag in bit 31, cached normal, sum x y z, 0;
//   fast    (rt_accum_create_fast, rt_fast_units.h): pixel, next sample, total x y z, open x y z;
//   moment  (rt_accum_create_fast_moments, rt_moments.h; a buffer of its own, one record per fast
//           record, whose `next` it shares): total2 x y z, open2 x y z, 0, 0.
// Word 1 is the next sample in both chain-buffer kinds, so the selection, mark and counts
// kernels read either through next_of.  Readers: rt_mega.h (parked, park_pixel, fast_rec,
// fast_rec_store, moment_rec, moment_rec_store, the LDS RNG word), rt_accum_device.h (next_of,
// rt_accum_state), rt_accum_file.h (read); tests/test_records.py checks the text against the
// records the Python tests build by hand.
#pragma once
#include <cstdint>

#include "rt_fast_units.h"

namespace rtrec {

constexpr int kWords = 8;
enum Word : int {
    kPixel = 0, kNext = 1,   // every chain-buffer record
    kParityState = 2, kParityCached = 3, kParitySum = 4, kParityZero = 7,
    kFastTotal = 2, kFastOpen = 5,
    kMomentTotal = 0, kMomentOpen = 3, kMomentZero = 6,
};

// A record by value (rt_mega.h loads and stores it as two 16-byte words).
struct Words {
    uint32_t w[kWords];
};

// The next sample of record p of a chain buffer of either kind.
RT_HD uint32_t next_of(const uint32_t *records, long long p) { return records[kWords * p + kNext]; }

// The engine word: the minstd state is below 2^31 (modulus 2^31 - 1), so the normal-cache flag
// (0 or 1) rides in its top bit (rt_device_selfcheck 1 checks the round trip).
RT_HD uint32_t rng_word_pack(uint32_t x, uint32_t saved_avail) { return x | saved_avail << 31; }
RT_HD void rng_word_unpack(uint32_t w, uint32_t &x, uint32_t &saved_avail) {
    x = w & 0x7fffffffu;
    saved_avail = w >> 31;
}

RT_HD void put3(uint32_t *w, const float *v) {
    for (int ch = 0; ch < 3; ++ch) w[ch] = rtm::f2u(v[ch]);
}
RT_HD void get3(const uint32_t *w, float *v) {
    for (int ch = 0; ch < 3; ++ch) v[ch] = rtm::u2f(w[ch]);
}

// A parity record: the state sample `next` starts from and the sum of the samples before it.
struct Parity {
    uint32_t pix, next, state, cached_avail;
    float cached, sum[3];
};
RT_HD Parity parity_unpack(const uint32_t *w) {
    Parity q;
    q.pix = w[kPixel];
    q.next = w[kNext];
    rng_word_unpack(w[kParityState], q.state, q.cached_avail);
    q.cached = rtm::u2f(w[kParityCached]);
    get3(w + kParitySum, q.sum);
    return q;
}
RT_HD void parity_pack(const Parity &q, uint32_t *w) {
    w[kPixel] = q.pix;
    w[kNext] = q.next;
    w[kParityState] = rng_word_pack(q.state, q.cached_avail);
    w[kParityCached] = rtm::f2u(q.cached);
    put3(w + kParitySum, q.sum);
    w[kParityZero] = 0u;
}

// A fast record: the pixel and the arithmetic part (rt_fast_units.h).
struct Fast {
    uint32_t pix;
    rtfu::Rec r;
};
RT_HD Fast fast_unpack(const uint32_t *w) {
    Fast q;
    q.pix = w[kPixel];
    q.r.next = (int)w[kNext];
    get3(w + kFastTotal, q.r.total);
    get3(w + kFastOpen, q.r.open);
    return q;
}
RT_HD void fast_pack(const Fast &q, uint32_t *w) {
    w[kPixel] = q.pix;
    w[kNext] = (uint32_t)q.r.next;
    put3(w + kFastTotal, q.r.total);
    put3(w + kFastOpen, q.r.open);
}

// A moment record: total2 and open2 of r; r.next is the fast record's and is not touched.
RT_HD void moment_unpack(const uint32_t *w, rtfu::Rec &r) {
    get3(w + kMomentTotal, r.total);
    get3(w + kMomentOpen, r.open);
}
RT_HD void moment_pack(const rtfu::Rec &r, uint32_t *w) {
    put3(w + kMomentTotal, r.total);
    put3(w + kMomentOpen, r.open);
    for (int k = kMomentZero; k < kWords; ++k) w[k] = 0u;
}

// Checkpoint checks over a whole record whose pixel stands at `next`: where no chunk is open, a
// fast record's open words are zero, and a moment record's open2 and pad words are.
RT_HD bool open_words_fit(uint32_t next, int c, const uint32_t *w) {
    return rtfu::open_words_fit(next, c, w + kFastOpen);
}
RT_HD bool record_words_fit(uint32_t next, int c, const uint32_t *w) {
    uint32_t any = 0u;
    for (int k = kMomentOpen; k < kWords; ++k) any |= w[k];
    return next % (uint32_t)c != 0u || any == 0u;
}

}  // namespace rtrec
