// records_host.cpp — TEST ONLY: rt_records.h (the accumulator's 32-byte per-pixel records) behind
// a C interface for tests/test_records.py.  Records are 8 words each; fields cross as words too,
// floats by their bits.  The header is host-clean, so this builds with plain g++.
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_records.h"

using namespace rtrec;

extern "C" {

int rh_words() { return kWords; }

unsigned rh_next_of(const unsigned *records, long long p) { return next_of(records, p); }

// Parity fields: pixel, next, state, flag, cached, sum x y z.
void rh_parity_unpack(long long n, const unsigned *w, unsigned *fields) {
    for (long long k = 0; k < n; ++k, w += kWords, fields += 8) {
        const Parity q = parity_unpack(w);
        const unsigned f[5] = {q.pix, q.next, q.state, q.cached_avail, rtm::f2u(q.cached)};
        std::memcpy(fields, f, sizeof f);
        put3(fields + 5, q.sum);
    }
}
void rh_parity_pack(long long n, const unsigned *fields, unsigned *w) {
    for (long long k = 0; k < n; ++k, w += kWords, fields += 8) {
        Parity q{fields[0], fields[1], fields[2], fields[3], rtm::u2f(fields[4]), {}};
        get3(fields + 5, q.sum);
        parity_pack(q, w);
    }
}

// Fast fields: pixel, next, total x y z, open x y z.
void rh_fast_unpack(long long n, const unsigned *w, unsigned *fields) {
    for (long long k = 0; k < n; ++k, w += kWords, fields += 8) {
        const Fast q = fast_unpack(w);
        fields[0] = q.pix;
        fields[1] = (unsigned)q.r.next;
        put3(fields + 2, q.r.total);
        put3(fields + 5, q.r.open);
    }
}
void rh_fast_pack(long long n, const unsigned *fields, unsigned *w) {
    for (long long k = 0; k < n; ++k, w += kWords, fields += 8) {
        Fast q;
        q.pix = fields[0];
        q.r.next = (int)fields[1];
        get3(fields + 2, q.r.total);
        get3(fields + 5, q.r.open);
        fast_pack(q, w);
    }
}

// Moment fields: total2 x y z, open2 x y z.
void rh_moment_unpack(long long n, const unsigned *w, unsigned *fields) {
    for (long long k = 0; k < n; ++k, w += kWords, fields += 6) {
        rtfu::Rec r;
        r.next = 0;
        moment_unpack(w, r);
        put3(fields, r.total);
        put3(fields + 3, r.open);
    }
}
void rh_moment_pack(long long n, const unsigned *fields, unsigned *w) {
    for (long long k = 0; k < n; ++k, w += kWords, fields += 6) {
        rtfu::Rec r;
        r.next = 0;
        get3(fields, r.total);
        get3(fields + 3, r.open);
        moment_pack(r, w);
    }
}

int rh_open_words_fit(unsigned next, int c, const unsigned *w) { return open_words_fit(next, c, w); }
int rh_record_words_fit(unsigned next, int c, const unsigned *w) { return record_words_fit(next, c, w); }

}  // extern "C"
