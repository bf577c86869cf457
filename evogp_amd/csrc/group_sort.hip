// group_sort.hip — the rocPRIM sorts and scans behind group_sort.hpp (gfx950): the only translation unit that instantiates them.
//
// The overloads and argument types are the ones dedup.hip, lexicase.hip and nsga2.hip called directly before (the double_buffer sort
// with a 32-bit size, the in/out sorts and the scans with size_t), so rocPRIM runs the kernels it ran for them.
#include "group_sort.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace evogp {

using u64 = unsigned long long;

static hipError_t raise(hipError_t e, size_t need, size_t *temp_bytes) {
    if (e == hipSuccess && need > *temp_bytes) *temp_bytes = need;
    return e;
}

// (the null iterators of a size query, typed as the calls below type theirs)
static const unsigned *const kIn32 = nullptr;
static unsigned *const kOut32 = nullptr;
static const u64 *const kIn64 = nullptr;
static u64 *const kOut64 = nullptr;

hipError_t sort_buffers_temp(unsigned n, size_t *temp_bytes) {
    size_t need = 0;
    rocprim::double_buffer<u64> kb(nullptr, nullptr);
    rocprim::double_buffer<unsigned> vb(nullptr, nullptr);
    return raise(rocprim::radix_sort_pairs(nullptr, need, kb, vb, n, 0, 64, (hipStream_t)0), need, temp_bytes);
}

hipError_t sort_pairs_u32_temp(unsigned n, size_t *temp_bytes) {
    size_t need = 0;
    return raise(rocprim::radix_sort_pairs(nullptr, need, kIn32, kOut32, kIn32, kOut32, (size_t)n, 0u, 32u, (hipStream_t)0), need, temp_bytes);
}

hipError_t sort_pairs_u64_temp(unsigned n, size_t *temp_bytes) {
    size_t need = 0;
    return raise(rocprim::radix_sort_pairs(nullptr, need, kIn64, kOut64, kIn32, kOut32, (size_t)n, 0u, 64u, (hipStream_t)0), need, temp_bytes);
}

hipError_t scan_max_temp(unsigned n, size_t *temp_bytes) {
    size_t need = 0;
    return raise(rocprim::inclusive_scan(nullptr, need, kIn32, kOut32, (size_t)n, rocprim::maximum<unsigned>(), (hipStream_t)0), need, temp_bytes);
}

hipError_t scan_plus_temp(unsigned n, size_t *temp_bytes) {
    size_t need = 0;
    return raise(rocprim::inclusive_scan(nullptr, need, kIn32, kOut32, (size_t)n, rocprim::plus<unsigned>(), (hipStream_t)0), need, temp_bytes);
}

hipError_t scan_plus_excl_temp(unsigned n, size_t *temp_bytes) {
    size_t need = 0;
    return raise(rocprim::exclusive_scan(nullptr, need, kIn32, kOut32, 0u, (size_t)n, rocprim::plus<unsigned>(), (hipStream_t)0), need, temp_bytes);
}

hipError_t sort_buffers(void *temp, size_t temp_bytes, u64 *keys_a, u64 *keys_b, unsigned *vals_a, unsigned *vals_b, unsigned n, bool *in_b,
                        hipStream_t stream) {
    rocprim::double_buffer<u64> kb(keys_a, keys_b);
    rocprim::double_buffer<unsigned> vb(vals_a, vals_b);
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, kb, vb, n, 0, 64, stream);
    *in_b = kb.current() == keys_b;
    return e;
}

hipError_t sort_pairs(void *temp, size_t temp_bytes, const unsigned *keys_in, unsigned *keys_out, const unsigned *vals_in, unsigned *vals_out,
                      unsigned n, unsigned begin_bit, unsigned end_bit, hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, begin_bit, end_bit, stream);
}

hipError_t sort_pairs(void *temp, size_t temp_bytes, const u64 *keys_in, u64 *keys_out, const unsigned *vals_in, unsigned *vals_out, unsigned n,
                      unsigned begin_bit, unsigned end_bit, hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, begin_bit, end_bit, stream);
}

hipError_t scan_max(void *temp, size_t temp_bytes, const unsigned *in, unsigned *out, unsigned n, hipStream_t stream) {
    return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)n, rocprim::maximum<unsigned>(), stream);
}

hipError_t scan_plus(void *temp, size_t temp_bytes, const unsigned *in, unsigned *out, unsigned n, hipStream_t stream) {
    return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)n, rocprim::plus<unsigned>(), stream);
}

hipError_t scan_plus_excl(void *temp, size_t temp_bytes, const unsigned *in, unsigned *out, unsigned n, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, 0u, (size_t)n, rocprim::plus<unsigned>(), stream);
}

} // namespace evogp
