// blob_io.hpp — what every stand-alone test program (tests/*_prog.cpp) needs around its own work: a reader over a little-endian blob, a
// writer that collects the output and checks the write, and the argument / exception handling of main.  Header only, C++14, the standard
// library alone.
#pragma once
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

struct BlobReader {
    std::vector<char> buf;
    size_t at = 0;
    explicit BlobReader(const char *path) {
        FILE *f = std::fopen(path, "rb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path);
        char tmp[1 << 16];
        size_t n;
        while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        std::fclose(f);
    }
    template <class T> void need(size_t n) const {                     // (no product of n: a hostile count cannot wrap it)
        if (n > (buf.size() - at) / sizeof(T)) throw std::runtime_error("input too short");
    }
    template <class T> void get(T *dst, size_t n) {
        need<T>(n);
        if (n) std::memcpy((void *)dst, buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
    }
    template <class T> T one() {
        T v;
        get(&v, 1);
        return v;
    }
    template <class T> std::vector<T> many(size_t n) {
        need<T>(n);                                                     // before the allocation
        std::vector<T> v(n);
        get(v.data(), n);
        return v;
    }
};

struct BlobWriter {
    std::vector<char> buf;
    template <class T> void put(const T *p, size_t n) {
        if (n) buf.insert(buf.end(), (const char *)p, (const char *)p + n * sizeof(T));
    }
    template <class T> void put(const std::vector<T> &v) { put(v.data(), v.size()); }
    void save(const char *path) const {
        FILE *f = std::fopen(path, "wb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path);
        const bool all = buf.empty() || std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
        if (std::fclose(f) != 0 || !all) throw std::runtime_error(std::string("short write to ") + path);
    }
};

struct BlobUsage {};                    // run throws it for an argument list it does not take

// main's body: `usage` begins with the program's name.  run(argc, argv) returns the exit code; BlobUsage -> 2 and the usage text, any
// std::exception -> 1 and "prog: what()".
template <class Run> int blob_main(int argc, char **argv, const char *usage, Run run) {
    try {
        return run(argc, argv);
    } catch (const BlobUsage &) {
        std::fprintf(stderr, "usage: %s\n", usage);
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%.*s: %s\n", (int)std::strcspn(usage, " "), usage, e.what());
        return 1;
    }
}
