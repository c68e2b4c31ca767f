// What the builders that sort on the device share (model.hip, layout_device.hip, reorder.hip, nmatrix.hip): rocprim's radix sorts and
// scan behind one call each (defined, and rocprim instantiated, in layout_device.hip only), their temporary storage, and the
// scratch of the layout builders.
#pragma once

#include "context.hpp"

namespace ipxk {

using u64 = unsigned long long;

inline int gridn(int64_t n) { return grid_for(n, 8192); }
inline int bits_for(u64 maxval) { int b = 1; while (b < 64 && (maxval >> b) != 0) b++; return b; }

struct Tmp {
    DevBuf<unsigned char> bytes;
    void* need(size_t n) { if (bytes.size() < n) bytes.resize(n); return bytes.get(); }
};
// stable sort of (key, value) pairs by the low `bits` bits of the key; K = unsigned or u64
template <class K>
void sort_pairs(Tmp& T, const K* kin, K* kout, const unsigned* vin, unsigned* vout, size_t n, int bits, hipStream_t s);
void sort_keys(Tmp& T, u64* in, u64* out, size_t n, hipStream_t s);       // by all 64 bits
void scan_int(Tmp& T, const int* in, int* out, size_t n, hipStream_t s);        // exclusive prefix sums
void narrow_ints(int64_t len, const ipxint* in, int* out, hipStream_t s);       // out[p] = (int)in[p] (model.hip)
void widen_ints(int64_t len, const int* in, ipxint* out, hipStream_t s);

// scratch of the layout builders: kept for the two gather matrices of a model, released when the model is built
struct LayoutScratch {
    DevBuf<unsigned> k1, k2, v1, v2, v3, v4;
    DevBuf<u64> q1, q2;
    DevBuf<int> stats;
    Tmp T;
};

}  // namespace ipxk
