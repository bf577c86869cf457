// group_sort.hpp — "sort by key, find the runs": the device-wide sorts and scans of dedup.hip, lexicase.hip and nsga2.hip.
//
// All of them are rocPRIM's; group_sort.hip is the one translation unit that includes rocPRIM and instantiates its kernels.  Every
// call works on the caller's stream out of the caller's temporary storage and returns rocPRIM's hipError_t; nothing synchronises
// with the host.  The sorts are stable.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace evogp {

// ---- temporary storage: raise *temp_bytes to what the primitive needs for n items (a caller folds the primitives it uses) ----------
hipError_t sort_buffers_temp(unsigned n, size_t *temp_bytes);
hipError_t sort_pairs_u32_temp(unsigned n, size_t *temp_bytes);
hipError_t sort_pairs_u64_temp(unsigned n, size_t *temp_bytes);
hipError_t scan_max_temp(unsigned n, size_t *temp_bytes);
hipError_t scan_plus_temp(unsigned n, size_t *temp_bytes);
hipError_t scan_plus_excl_temp(unsigned n, size_t *temp_bytes);

// ---- sorts -----------------------------------------------------------------------------------------------------------------------
// (u64 key, u32 value) pairs on all 64 bits, from keys_a / vals_a, ping-ponging between the two sides; *in_b: the result is in
// keys_b / vals_b (else in keys_a / vals_a), the other side holds garbage
hipError_t sort_buffers(void *temp, size_t temp_bytes, unsigned long long *keys_a, unsigned long long *keys_b, unsigned *vals_a, unsigned *vals_b,
                        unsigned n, bool *in_b, hipStream_t stream);
// pairs on the key bits [begin_bit, end_bit), from the in arrays into the out arrays
hipError_t sort_pairs(void *temp, size_t temp_bytes, const unsigned *keys_in, unsigned *keys_out, const unsigned *vals_in, unsigned *vals_out,
                      unsigned n, unsigned begin_bit, unsigned end_bit, hipStream_t stream);
hipError_t sort_pairs(void *temp, size_t temp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out, const unsigned *vals_in,
                      unsigned *vals_out, unsigned n, unsigned begin_bit, unsigned end_bit, hipStream_t stream);

// ---- scans over n unsigned words --------------------------------------------------------------------------------------------------
hipError_t scan_max(void *temp, size_t temp_bytes, const unsigned *in, unsigned *out, unsigned n, hipStream_t stream);         // inclusive maximum
hipError_t scan_plus(void *temp, size_t temp_bytes, const unsigned *in, unsigned *out, unsigned n, hipStream_t stream);        // inclusive sum
hipError_t scan_plus_excl(void *temp, size_t temp_bytes, const unsigned *in, unsigned *out, unsigned n, hipStream_t stream);   // exclusive sum from 0

} // namespace evogp
