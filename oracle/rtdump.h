// rtdump.h — tiny named-array container used by the oracle tools to exchange golden
// vectors with the Python tests (reader: tests/rtdump.py).  TEST INFRASTRUCTURE ONLY.
//
// Layout: "RTD1", then records {u32 name_len, name, u8 dtype, u8 ndim, u64 shape[ndim],
// raw little-endian data}, terminated by name_len == 0.
// dtype: 'f' f32, 'd' f64, 'i' i32, 'I' u32, 'q' i64, 'Q' u64, 'B' u8.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

class RtDump {
public:
    explicit RtDump(const std::string &path) {
        f_ = std::fopen(path.c_str(), "wb");
        if (!f_) throw std::runtime_error("rtdump: cannot open " + path);
        std::fwrite("RTD1", 1, 4, f_);
    }
    ~RtDump() { close(); }
    void close() {
        if (!f_) return;
        uint32_t z = 0;
        std::fwrite(&z, 4, 1, f_);
        std::fclose(f_);
        f_ = nullptr;
    }
    template <class T>
    void put(const std::string &name, const std::vector<T> &v, std::vector<uint64_t> shape = {}) {
        if (shape.empty()) shape.push_back(v.size());
        put_raw(name, code<T>(), shape, v.data(), v.size() * sizeof(T));
    }
    template <class T>
    void scalar(const std::string &name, T v) { put_raw(name, code<T>(), {1}, &v, sizeof(T)); }

private:
    template <class T> static char code();
    void put_raw(const std::string &name, char dt, const std::vector<uint64_t> &shape, const void *p, size_t n) {
        uint32_t len = (uint32_t)name.size();
        std::fwrite(&len, 4, 1, f_);
        std::fwrite(name.data(), 1, len, f_);
        uint8_t d = (uint8_t)dt, nd = (uint8_t)shape.size();
        std::fwrite(&d, 1, 1, f_);
        std::fwrite(&nd, 1, 1, f_);
        std::fwrite(shape.data(), 8, shape.size(), f_);
        if (n) std::fwrite(p, 1, n, f_);
    }
    std::FILE *f_ = nullptr;
};
template <> inline char RtDump::code<float>() { return 'f'; }
template <> inline char RtDump::code<double>() { return 'd'; }
template <> inline char RtDump::code<int32_t>() { return 'i'; }
template <> inline char RtDump::code<uint32_t>() { return 'I'; }
template <> inline char RtDump::code<int64_t>() { return 'q'; }
template <> inline char RtDump::code<uint64_t>() { return 'Q'; }
template <> inline char RtDump::code<uint8_t>() { return 'B'; }

// Reads the array `name` of an RTD1 file: 4-byte items of dtype `want` ('f' or 'I'), shape (n, cols),
// or (n) where cols is 0.  Every length in the file is checked against the file's size before it is used.
inline std::vector<uint32_t> rtdump_read_words(const std::string &path, const std::string &name, char want, uint64_t cols) {
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("rtdump: cannot open " + path);
    std::vector<uint8_t> buf;
    uint8_t chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    size_t p = 4;
    auto need = [&](uint64_t n) {
        if (n > buf.size() || p > buf.size() - n) throw std::runtime_error("rtdump: truncated " + path);
    };
    if (buf.size() < 4 || std::memcmp(buf.data(), "RTD1", 4) != 0) throw std::runtime_error("rtdump: not an RTD1 file: " + path);
    for (;;) {
        need(4);
        uint32_t len;
        std::memcpy(&len, &buf[p], 4);
        p += 4;
        if (len == 0) break;
        need((uint64_t)len + 2);
        const std::string nm((const char *)&buf[p], len);
        p += len;
        const uint8_t dt = buf[p], nd = buf[p + 1];
        p += 2;
        need(8ull * nd);
        std::vector<uint64_t> shape(nd);
        if (nd) std::memcpy(shape.data(), &buf[p], 8ull * nd);
        p += 8ull * nd;
        uint64_t count = 1;
        for (uint64_t d : shape) {
            if (d != 0 && count > buf.size() / d) throw std::runtime_error("rtdump: truncated " + path);
            count *= d;
        }
        const uint64_t item = (dt == 'd' || dt == 'q' || dt == 'Q') ? 8 : (dt == 'B' ? 1 : 4);
        if (count > buf.size() / item) throw std::runtime_error("rtdump: truncated " + path);
        need(count * item);
        if (nm == name) {
            if (dt != (uint8_t)want || (cols ? (nd != 2 || shape[1] != cols) : nd != 1))
                throw std::runtime_error("rtdump: " + name + " has another type or shape than asked for");
            std::vector<uint32_t> out(count);
            if (count) std::memcpy(out.data(), &buf[p], count * 4);
            return out;
        }
        p += count * item;
    }
    throw std::runtime_error("rtdump: no array " + name + " in " + path);
}
inline std::vector<float> rtdump_read_f32(const std::string &path, const std::string &name, uint64_t cols) {
    const std::vector<uint32_t> w = rtdump_read_words(path, name, 'f', cols);
    std::vector<float> out(w.size());
    if (!w.empty()) std::memcpy(out.data(), w.data(), w.size() * 4);
    return out;
}
inline std::vector<uint32_t> rtdump_read_u32(const std::string &path, const std::string &name) {
    return rtdump_read_words(path, name, 'I', 0);
}
