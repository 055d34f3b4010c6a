// blob_io_prog.cpp — tests/blob_io.hpp on its own, for tests/test_blob_io.py (built through tests/host_prog.py, plain and under the
// sanitizers): `blob_io_prog copy IN OUT` reads five arrays and writes them back in the same layout, so OUT equals IN byte for byte.
//   IN, OUT: i64 n, u8[n]; i64 n, i32[n]; i64 n, i64[n]; i64 n, f32[n]; i64 n, f64[n]
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"

template <class T> static void copy_many(BlobReader &r, BlobWriter &w) {       // many() and put(vector)
    const int64_t n = r.one<int64_t>();
    const std::vector<T> v = r.many<T>((size_t)n);
    w.put(&n, 1);
    w.put(v);
}

template <class T> static void copy_get(BlobReader &r, BlobWriter &w) {        // need() then get() into a caller's buffer, and put(p, n)
    const int64_t n = r.one<int64_t>();
    r.need<T>((size_t)n);
    std::vector<T> v((size_t)n);
    r.get(v.data(), v.size());
    w.put(&n, 1);
    w.put(v.data(), v.size());
}

static int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "copy") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    copy_many<uint8_t>(r, w);
    copy_get<int32_t>(r, w);
    copy_many<int64_t>(r, w);
    copy_get<float>(r, w);
    copy_many<double>(r, w);
    if (r.at != r.buf.size()) throw std::runtime_error("input too long");
    w.save(argv[3]);
    return 0;
}

int main(int argc, char **argv) { return blob_main(argc, argv, "blob_io_prog copy IN OUT", run); }
