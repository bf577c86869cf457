// torch_ops.cpp — libtorch registration of the operator boundary: TORCH_LIBRARY(evogp_cuda) with the reference's five
// schemas verbatim (src/evogp/cuda/torch_wrapper.cu:291-299) and their CUDA-key implementations (:301-307; ROCm builds of
// PyTorch dispatch HIP tensors on the CUDA key), plus the extra ops of this engine in the evogp_hip namespace.
//
// Each implementation does what the reference's wrapper does — validate the sizes (torch_wrapper.cu:48-54,103-104,154-156,
// 205-208,250-254), require contiguous device tensors of the exact shape (check_tensor, :7-17), allocate the outputs on the
// device of the designated input (:63,116,168,217,264) — and then calls the C ABI of include/evogp_hip.h with raw device
// pointers on torch's CURRENT stream of that device (the reference launches on the legacy default stream).  Differences:
// dtypes are checked explicitly (the reference relies on data_ptr<T>()), every tensor must live on the same device, and
// launch errors are reported (the reference's check_cuda_error calls are commented out, :84,135,188,231,282).
//
// The ops are built from a few parts: Forest (a checked (value, type, size) triple with its sizes, device and typed pointers),
// check_dataset (the prologue of the ops over a dataset), ForestOut (a fresh forest and its pointers) and Donors (the donor rows of
// the row-range breed ops).  An op body is then: its own checks, its outputs, one C call, check_rc.  Every check comes before the
// first allocation.
//
// Host code only (no kernels): compiled with g++ against the torch headers and linked to libevogp_hip.so.  There is no CPU
// implementation and no fallback: a CPU tensor fails in the dispatcher exactly as with the reference.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>

#include "../../include/evogp_hip.h"

namespace {

using at::Tensor;
using Tensor3 = std::tuple<Tensor, Tensor, Tensor>;
using Tensor4 = std::tuple<Tensor, Tensor, Tensor, Tensor>;

constexpr int64_t kMaxStack = EVOGP_MAX_STACK;

// `name` `suffix` is what an error text calls the tensor ("value" "_ori"); the text is put together only when a check fails
void check_tensor(const Tensor &t, at::IntArrayRef shape, const char *name, const c10::Device &dev,
                  c10::optional<at::ScalarType> dtype = c10::nullopt, const char *suffix = "") {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, suffix, " must be a contiguous CUDA tensor");
    TORCH_CHECK(t.device() == dev, name, suffix, " lives on ", t.device(), " but the call runs on ", dev,
                ": all operands of one call must share a device");
    TORCH_CHECK(t.sizes() == shape, name, suffix, " must have shape ", shape, ", but got shape ", t.sizes());
    if (dtype) TORCH_CHECK(t.scalar_type() == *dtype, "expected scalar type ", *dtype, " for ", name, suffix, " but found ", t.scalar_type());
}

void check_sizes(int64_t pop_size, int64_t gp_len) {
    TORCH_CHECK(pop_size > 0, "pop_size must be larger than 0, but got ", pop_size);
    TORCH_CHECK(gp_len > 0 && gp_len <= kMaxStack, "gp_len must be in range (0, ", kMaxStack, "], but got ", gp_len);
}

void check_rc(int rc, const char *what) {
    TORCH_CHECK(rc == 0, what, " failed: ", evogp_hip_error_string(rc), " (code ", rc, ")");
}

// torch's current stream of the device.  (ROCm builds of torch present their devices as DeviceType::CUDA; the generic
// c10::DeviceGuard resolves to the registered implementation, and the stream pool is indexed by the device ordinal.)
evogp_stream_t current_stream(const c10::Device &dev) { return (evogp_stream_t)c10::hip::getCurrentHIPStream(dev.index()).stream(); }

Tensor empty(at::IntArrayRef shape, at::ScalarType dtype, const c10::Device &dev) {
    return at::empty(shape, at::TensorOptions().dtype(dtype).device(dev));
}

// A checked forest: three contiguous (pop, gp_len) tensors float32 / int16 / int16 on one device.  The sizes are the caller's, or
// those of `value` (infer; at most 2^31 - 1 rows, for every op that infers); the device is the caller's (`on`), or that of `value`.
// A forest that goes WITH another one (donors) has no size rule of its own, only the shape: it may have no rows at all.
struct Forest {
    int64_t pop, gp_len;
    c10::Device dev;
    float *value;
    int16_t *type, *size;

    Forest(int64_t pop_size, int64_t gp_len_, const Tensor &v, const Tensor &t, const Tensor &s, const char *suffix = "",
           const c10::Device *on = nullptr, bool goes_with_another = false)
        : pop(pop_size), gp_len(gp_len_), dev(on ? *on : v.device()) {
        if (!goes_with_another) check_sizes(pop, gp_len);
        check_tensor(v, {pop, gp_len}, "value", dev, at::kFloat, suffix);
        check_tensor(t, {pop, gp_len}, "type", dev, at::kShort, suffix);
        check_tensor(s, {pop, gp_len}, "subtree_size", dev, at::kShort, suffix);
        value = v.data_ptr<float>(), type = t.data_ptr<int16_t>(), size = s.data_ptr<int16_t>();
    }

    static Forest infer(const Tensor &v, const Tensor &t, const Tensor &s) {
        TORCH_CHECK(v.dim() == 2, "value must be a (pop_size, gp_len) tensor");
        TORCH_CHECK(v.size(0) <= 0x7FFFFFFF, "too many trees: ", v.size(0));
        return Forest(v.size(0), v.size(1), v, t, s);
    }
    // `rows` donor rows for a forest on `dev` (rows >= 0: an all-elite range or generation has no offspring)
    static Forest donors(int64_t rows, int64_t gp_len, const Tensor &v, const Tensor &t, const Tensor &s, const c10::Device &dev) {
        return Forest(rows, gp_len, v, t, s, " (donor)", &dev, true);
    }
};

// A fresh forest of `rows` rows on `dev` and its typed pointers.
struct ForestOut {
    Tensor tv, tt, ts;
    float *value;
    int16_t *type, *size;

    ForestOut(int64_t rows, int64_t gp_len, const c10::Device &dev)
        : tv(empty({rows, gp_len}, at::kFloat, dev)), tt(empty({rows, gp_len}, at::kShort, dev)), ts(empty({rows, gp_len}, at::kShort, dev)),
          value(tv.data_ptr<float>()), type(tt.data_ptr<int16_t>()), size(ts.data_ptr<int16_t>()) {}

    Tensor3 tuple() const { return {tv, tt, ts}; }
    Tensor4 with(const Tensor &fourth) const { return {tv, tt, ts, fourth}; }
};

// The prologue of the ops over a dataset: the forest, the sizes, variables (data_points, var_len) and labels (data_points, out_len);
// `op` is the op's name for its error texts.
enum class OutLen { Any, One, UpTo16, Genes };   // what the op allows: any positive out_len, single-output trees only, the output registers,
                                                 // 1..EVOGP_GENES_MAX features of ONE label column

struct Dataset : Forest {
    const float *X, *y;
};

Dataset check_dataset(const char *op, OutLen rule, int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                      const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(var_len > 0, "var_len must be larger than 0, but got ", var_len);
    switch (rule) {
    case OutLen::Any: TORCH_CHECK(out_len > 0, "out_len must be larger than 0, but got ", out_len); break;
    case OutLen::One: TORCH_CHECK(out_len == 1, op, ": single-output trees only (out_len must be 1), but got ", out_len); break;
    case OutLen::UpTo16: TORCH_CHECK(out_len > 0 && out_len <= 16, "out_len must be in range (0, 16], but got ", out_len); break;
    case OutLen::Genes: TORCH_CHECK(out_len > 0 && out_len <= EVOGP_GENES_MAX, "out_len must be in range (0, ", EVOGP_GENES_MAX, "], but got ", out_len); break;
    }
    TORCH_CHECK(data_points > 0, "data_points must be larger than 0, but got ", data_points);
    check_tensor(variables, {data_points, var_len}, "variables", f.dev, at::kFloat);
    if (rule == OutLen::Genes && labels.dim() == 1) check_tensor(labels, {data_points}, "labels", f.dev, at::kFloat);   // (D,) or (D, 1)
    else check_tensor(labels, {data_points, rule == OutLen::Genes ? 1 : out_len}, "labels", f.dev, at::kFloat);
    return {f, variables.data_ptr<float>(), labels.data_ptr<float>()};
}

// The donor rows of the row-range breed ops.  The donor arrays are aligned with the OFFSPRING rows of the range: they may cover the
// whole range (row_count rows; the rows of elites are never read) or only its offspring (row_count minus the elite rows at the head
// of the range) -- then no padding copy is needed.  The engine indexes donors by (row - row_begin), so the pointers are rewound by
// the rows that are left out.
struct Donors {
    const float *value;
    const int16_t *type, *size;

    Donors(const Tensor &v, const Tensor &t, const Tensor &s, int64_t row_begin, int64_t row_count, int64_t n_elite, int64_t gp_len,
           const c10::Device &dev) {
        const int64_t head = std::max<int64_t>(0, std::min(row_begin + row_count, n_elite) - row_begin);  // elite rows at the head of the range
        const int64_t drows = v.dim() == 2 ? v.size(0) : -1;
        TORCH_CHECK(drows == row_count || drows == row_count - head, "donor arrays must have ", row_count, " or ", row_count - head,
                    " rows, but got ", drows);
        const Forest f = Forest::donors(drows, gp_len, v, t, s, dev);
        const int64_t skip = drows == row_count - head ? head : 0;
        value = f.value - skip * gp_len, type = f.type - skip * gp_len, size = f.size - skip * gp_len;
    }
};

// the reference reads keys.data_ptr<unsigned int>() (torch_wrapper.cu:76); signed integer keys carry the same 32-bit patterns
Tensor keys_u32(const Tensor &keys) {
    if (keys.scalar_type() == at::kUInt32) return keys;
    TORCH_CHECK(keys.scalar_type() == at::kInt || keys.scalar_type() == at::kLong, "keys must be uint32/int32/int64, got ", keys.scalar_type());
    return keys.to(at::kLong).bitwise_and(0xFFFFFFFFLL).to(at::kUInt32).contiguous();
}

// what the three generators check: the sizes, the probabilities, the 32-bit arguments and the three tables (on the device of the first)
void check_generate(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, int64_t const_samples_len, double out_prob,
                    double const_prob, int64_t tree_index_offset, int64_t active_below, const Tensor &depth2leaf_probs,
                    const Tensor &roulette_funcs, const Tensor &const_samples, const c10::Device &dev) {
    check_sizes(pop_size, gp_len);
    TORCH_CHECK(var_len > 0, "var_len must be larger than 0, but got ", var_len);
    TORCH_CHECK(out_len > 0, "out_len must be larger than 0, but got ", out_len);
    TORCH_CHECK(const_samples_len > 0, "const_samples_len must be larger than 0, but got ", const_samples_len);
    TORCH_CHECK(out_prob >= 0 && out_prob <= 1, "out_prob must be in range [0, 1], but got ", out_prob);
    TORCH_CHECK(const_prob >= 0 && const_prob <= 1, "const_prob must be in range [0, 1], but got ", const_prob);
    TORCH_CHECK(tree_index_offset >= 0 && tree_index_offset < (1LL << 32), "tree_index_offset must fit in 32 bits");
    TORCH_CHECK(active_below >= 0 && active_below < (1LL << 32), "active_below must fit in 32 bits");
    check_tensor(depth2leaf_probs, {EVOGP_MAX_FULL_DEPTH}, "depth2leaf_probs", dev, at::kFloat);
    check_tensor(roulette_funcs, {EVOGP_NUM_FUNCS}, "roulette_funcs", dev, at::kFloat);
    check_tensor(const_samples, {const_samples_len}, "const_samples", dev, at::kFloat);
}

Tensor3 generate_impl(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, int64_t const_samples_len, double out_prob,
                      double const_prob, const Tensor &keys_in, const Tensor &depth2leaf_probs, const Tensor &roulette_funcs,
                      const Tensor &const_samples, int64_t tree_index_offset, const Tensor *active_word, int64_t active_below) {
    const c10::Device dev = keys_in.device();
    check_generate(pop_size, gp_len, var_len, out_len, const_samples_len, out_prob, const_prob, tree_index_offset, active_below,
                   depth2leaf_probs, roulette_funcs, const_samples, dev);
    check_tensor(keys_in, {2}, "keys", dev);
    if (active_word) check_tensor(*active_word, {pop_size}, "active_word", dev, at::kInt);
    const Tensor keys = keys_u32(keys_in);
    c10::DeviceGuard guard(dev);
    const ForestOut out(pop_size, gp_len, dev);
    check_rc(evogp_hip_generate_masked((unsigned)pop_size, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, (unsigned)const_samples_len,
                                       (float)out_prob, (float)const_prob, (const unsigned *)keys.data_ptr(), depth2leaf_probs.data_ptr<float>(),
                                       roulette_funcs.data_ptr<float>(), const_samples.data_ptr<float>(), out.value, out.type, out.size,
                                       (unsigned)tree_index_offset, active_word ? active_word->data_ptr<int>() : nullptr, (unsigned)active_below,
                                       current_stream(dev)),
             "tree_generate");
    return out.tuple();
}

// rows of trees whose counter-based word (4, n + tree_index_offset) of (seed, generation) is not below active_below are left
// uninitialised; no keys / active_word tensors (include/evogp_hip.h evogp_hip_generate_masked_hashed)
Tensor3 tree_generate_masked_hashed(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, int64_t const_samples_len, double out_prob,
                                    double const_prob, const Tensor &depth2leaf_probs, const Tensor &roulette_funcs, const Tensor &const_samples,
                                    int64_t tree_index_offset, int64_t seed, int64_t generation, int64_t active_below) {
    const c10::Device dev = depth2leaf_probs.device();
    check_generate(pop_size, gp_len, var_len, out_len, const_samples_len, out_prob, const_prob, tree_index_offset, active_below,
                   depth2leaf_probs, roulette_funcs, const_samples, dev);
    c10::DeviceGuard guard(dev);
    const ForestOut out(pop_size, gp_len, dev);
    check_rc(evogp_hip_generate_masked_hashed((unsigned)pop_size, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, (unsigned)const_samples_len,
                                              (float)out_prob, (float)const_prob, depth2leaf_probs.data_ptr<float>(), roulette_funcs.data_ptr<float>(),
                                              const_samples.data_ptr<float>(), out.value, out.type, out.size, (unsigned)tree_index_offset, seed,
                                              generation, (unsigned)active_below, current_stream(dev)),
             "tree_generate_masked_hashed");
    return out.tuple();
}

// ---- the reference's five ops -------------------------------------------------------------------------------------------
Tensor3 tree_generate(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, int64_t const_samples_len, double out_prob,
                      double const_prob, const Tensor &keys, const Tensor &depth2leaf_probs, const Tensor &roulette_funcs,
                      const Tensor &const_samples) {
    return generate_impl(pop_size, gp_len, var_len, out_len, const_samples_len, out_prob, const_prob, keys, depth2leaf_probs,
                         roulette_funcs, const_samples, 0, nullptr, 0);
}

Tensor3 tree_mutate(int64_t pop_size, int64_t gp_len, const Tensor &value_ori, const Tensor &type_ori, const Tensor &size_ori,
                    const Tensor &mutate_indices, const Tensor &value_new, const Tensor &type_new, const Tensor &size_new) {
    const c10::Device dev = value_new.device();
    const Forest ori(pop_size, gp_len, value_ori, type_ori, size_ori, "_ori", &dev);
    check_tensor(mutate_indices, {pop_size}, "mutateIndices", dev, at::kInt);
    const Forest fresh(pop_size, gp_len, value_new, type_new, size_new, "_new");
    c10::DeviceGuard guard(dev);
    const ForestOut out(pop_size, gp_len, dev);
    check_rc(evogp_hip_mutate((int)pop_size, (int)gp_len, ori.value, ori.type, ori.size, mutate_indices.data_ptr<int>(), fresh.value, fresh.type,
                              fresh.size, out.value, out.type, out.size, current_stream(dev)),
             "tree_mutate");
    return out.tuple();
}

Tensor3 tree_crossover(int64_t pop_size_ori, int64_t pop_size_new, int64_t gp_len, const Tensor &value_ori, const Tensor &type_ori,
                       const Tensor &size_ori, const Tensor &left_idx, const Tensor &right_idx, const Tensor &left_node_idx,
                       const Tensor &right_node_idx) {
    TORCH_CHECK(pop_size_ori > 0, "pop_size_ori must be larger than 0, but got ", pop_size_ori);
    TORCH_CHECK(pop_size_new > 0, "pop_size_new must be larger than 0, but got ", pop_size_new);
    const Forest ori(pop_size_ori, gp_len, value_ori, type_ori, size_ori, "_ori");
    const c10::Device dev = ori.dev;
    check_tensor(left_idx, {pop_size_new}, "left_idx", dev, at::kInt);
    check_tensor(right_idx, {pop_size_new}, "right_idx", dev, at::kInt);
    check_tensor(left_node_idx, {pop_size_new}, "left_node_idx", dev, at::kInt);
    check_tensor(right_node_idx, {pop_size_new}, "right_node_idx", dev, at::kInt);
    c10::DeviceGuard guard(dev);
    const ForestOut out(pop_size_new, gp_len, dev);
    check_rc(evogp_hip_crossover((int)pop_size_ori, (int)pop_size_new, (int)gp_len, ori.value, ori.type, ori.size, left_idx.data_ptr<int>(),
                                 right_idx.data_ptr<int>(), left_node_idx.data_ptr<int>(), right_node_idx.data_ptr<int>(), out.value, out.type,
                                 out.size, current_stream(dev)),
             "tree_crossover");
    return out.tuple();
}

Tensor tree_evaluate(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value, const Tensor &type,
                     const Tensor &size, const Tensor &variables) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(var_len > 0, "var_len must be larger than 0, but got ", var_len);
    TORCH_CHECK(out_len > 0, "out_len must be larger than 0, but got ", out_len);
    check_tensor(variables, {pop_size, var_len}, "variables", f.dev, at::kFloat);
    c10::DeviceGuard guard(f.dev);
    Tensor results = empty({pop_size, out_len}, at::kFloat, f.dev);
    check_rc(evogp_hip_evaluate((unsigned)pop_size, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value, f.type, f.size,
                                variables.data_ptr<float>(), results.data_ptr<float>(), current_stream(f.dev)),
             "tree_evaluate");
    return results;
}

Tensor sr_fitness_impl(const char *op, int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, bool use_mse,
                       const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels,
                       int64_t kernel_type, int64_t func_mask = 0) {
    const Dataset d = check_dataset(op, OutLen::Any, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    TORCH_CHECK(kernel_type >= 0 && kernel_type <= 4, "kernel_type must be in 0..4, but got ", kernel_type);
    TORCH_CHECK(func_mask >= 0 && func_mask < (1LL << 32), "func_mask must fit in 32 bits");
    c10::DeviceGuard guard(d.dev);
    Tensor fitness = empty({pop_size}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_fitness_hinted((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len,
                                         use_mse ? 1 : 0, d.value, d.type, d.size, d.X, d.y, fitness.data_ptr<float>(), (unsigned)kernel_type,
                                         (unsigned)func_mask, current_stream(d.dev)),
             op);
    return fitness;
}

Tensor tree_SR_fitness(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, bool use_mse,
                       const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels,
                       int64_t kernel_type) {
    return sr_fitness_impl("tree_SR_fitness", pop_size, data_points, gp_len, var_len, out_len, use_mse, value, type, size, variables, labels, kernel_type);
}

// tree_SR_fitness for a caller that knows the set of functions that can occur in the forest (0: unknown) -- include/evogp_hip.h
Tensor tree_SR_fitness_masked(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, bool use_mse,
                              const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels,
                              int64_t kernel_type, int64_t func_mask) {
    return sr_fitness_impl("tree_SR_fitness_masked", pop_size, data_points, gp_len, var_len, out_len, use_mse, value, type, size, variables, labels, kernel_type,
                           func_mask);
}

// ---- extra ops (no counterpart in the reference) ------------------------------------------------------------------------
// loss and d loss / d constant of every tree (include/evogp_hip.h evogp_hip_sr_gradient), validated like tree_SR_fitness
std::tuple<Tensor, Tensor> tree_SR_gradient(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, bool use_mse,
                                            const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                            const Tensor &labels) {
    const Dataset d = check_dataset("tree_SR_gradient", OutLen::UpTo16, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size}, at::kFloat, d.dev), grad = empty({pop_size, gp_len}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_gradient((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, use_mse ? 1 : 0,
                                   d.value, d.type, d.size, d.X, d.y, loss.data_ptr<float>(), grad.data_ptr<float>(), current_stream(d.dev)),
             "tree_SR_gradient");
    return {loss, grad};
}

// the loss of every subtree as a model of its own and its value where it is constant over the rows (evogp_hip_sr_subtree_errors)
std::tuple<Tensor, Tensor> tree_SR_subtree_errors(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                                  bool use_mse, const Tensor &value, const Tensor &type, const Tensor &size,
                                                  const Tensor &variables, const Tensor &labels) {
    const Dataset d = check_dataset("tree_SR_subtree_errors", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    c10::DeviceGuard guard(d.dev);
    Tensor node_err = empty({pop_size, gp_len}, at::kFloat, d.dev), node_const = empty({pop_size, gp_len}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_subtree_errors((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len,
                                         use_mse ? 1 : 0, d.value, d.type, d.size, d.X, d.y, node_err.data_ptr<float>(),
                                         node_const.data_ptr<float>(), current_stream(d.dev)),
             "tree_SR_subtree_errors");
    return {node_err, node_const};
}

// the loss and the coefficients of every tree under linear scaling (evogp_hip_sr_linear_scaling): loss (pop,), coef (pop, 2) = intercept, slope
std::tuple<Tensor, Tensor> tree_SR_linear_scaling(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                                  const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                  const Tensor &labels) {
    const Dataset d = check_dataset("tree_SR_linear_scaling", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size}, at::kFloat, d.dev), coef = empty({pop_size, 2}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_linear_scaling((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, d.value,
                                         d.type, d.size, d.X, d.y, loss.data_ptr<float>(), coef.data_ptr<float>(), current_stream(d.dev)),
             "tree_SR_linear_scaling");
    return {loss, coef};
}

// the weight rows of the weighted scoring passes: (K, data_points) float32 on the dataset's device with 1 <= K <= 8, or nullptr and
// K = 1 without them
static const float *weight_rows(const c10::optional<Tensor> &weights, int64_t data_points, const Dataset &d, int64_t *K) {
    *K = 1;
    if (!weights.has_value()) return nullptr;
    TORCH_CHECK(weights->dim() == 2 && weights->size(0) >= 1 && weights->size(0) <= EVOGP_WLOSS_MAX_WEIGHTS,
                "weights must be a (K, data_points) tensor with K in range [1, ", EVOGP_WLOSS_MAX_WEIGHTS, "], but got shape ", weights->sizes());
    *K = weights->size(0);
    check_tensor(*weights, {*K, data_points}, "weights", d.dev, at::kFloat);
    return weights->data_ptr<float>();
}

// weighted / robust / held-out losses (evogp_hip_sr_weighted_loss): loss (pop, K) for weights (K, D), (pop, 1) without weights
Tensor tree_SR_weighted_loss(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                             const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels,
                             const c10::optional<Tensor> &weights, int64_t loss_kind, double loss_param) {
    const Dataset d = check_dataset("tree_SR_weighted_loss", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    TORCH_CHECK(loss_kind >= EVOGP_LOSS_MSE && loss_kind <= EVOGP_LOSS_LOGCOSH, "loss_kind must be in range [", EVOGP_LOSS_MSE, ", ",
                EVOGP_LOSS_LOGCOSH, "], but got ", loss_kind);
    TORCH_CHECK(loss_param == loss_param, "loss_param must not be NaN");
    TORCH_CHECK(loss_kind != EVOGP_LOSS_HUBER || (loss_param > 0.0 && loss_param < HUGE_VAL),
                "loss_param (the delta of the Huber loss) must be finite and larger than 0, but got ", loss_param);
    TORCH_CHECK(loss_kind != EVOGP_LOSS_PINBALL || (loss_param > 0.0 && loss_param < 1.0),
                "loss_param (the tau of the pinball loss) must lie in (0, 1), but got ", loss_param);
    int64_t K = 1;
    const float *w = weight_rows(weights, data_points, d, &K);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size, K}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_weighted_loss((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, d.value,
                                        d.type, d.size, d.X, d.y, w, (unsigned)K, (int)loss_kind, loss_param, loss.data_ptr<float>(),
                                        current_stream(d.dev)),
             "tree_SR_weighted_loss");
    return loss;
}

// linear scaling fitted on weight row 0 and scored on every row (evogp_hip_sr_weighted_scaling): loss (pop, K) for weights (K, D),
// (pop, 1) without weights; coef (pop, 2) = intercept, slope
std::tuple<Tensor, Tensor> tree_SR_weighted_scaling(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                                    const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                    const Tensor &labels, const c10::optional<Tensor> &weights) {
    const Dataset d = check_dataset("tree_SR_weighted_scaling", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    int64_t K = 1;
    const float *w = weight_rows(weights, data_points, d, &K);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size, K}, at::kFloat, d.dev), coef = empty({pop_size, 2}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_weighted_scaling((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len,
                                           d.value, d.type, d.size, d.X, d.y, w, (unsigned)K, loss.data_ptr<float>(), coef.data_ptr<float>(),
                                           current_stream(d.dev)),
             "tree_SR_weighted_scaling");
    return {loss, coef};
}

// the one weight row of the weighted tuning passes: (data_points,) float32 on the dataset's device, or nullptr without one
static const float *weight_row(const c10::optional<Tensor> &weights, int64_t data_points, const Dataset &d) {
    if (!weights.has_value()) return nullptr;
    check_tensor(*weights, {data_points}, "weights", d.dev, at::kFloat);
    return weights->data_ptr<float>();
}

// loss and gradient under a weight row and one of the five losses (evogp_hip_sr_weighted_gradient): what tree_SR_weighted_loss scores by
std::tuple<Tensor, Tensor> tree_SR_weighted_gradient(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                                     const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                     const Tensor &labels, const c10::optional<Tensor> &weights, int64_t loss_kind,
                                                     double loss_param) {
    const Dataset d = check_dataset("tree_SR_weighted_gradient", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    TORCH_CHECK(loss_kind >= EVOGP_LOSS_MSE && loss_kind <= EVOGP_LOSS_LOGCOSH, "loss_kind must be in range [", EVOGP_LOSS_MSE, ", ",
                EVOGP_LOSS_LOGCOSH, "], but got ", loss_kind);
    TORCH_CHECK(loss_param == loss_param, "loss_param must not be NaN");
    TORCH_CHECK(loss_kind != EVOGP_LOSS_HUBER || (loss_param > 0.0 && loss_param < HUGE_VAL),
                "loss_param (the delta of the Huber loss) must be finite and larger than 0, but got ", loss_param);
    TORCH_CHECK(loss_kind != EVOGP_LOSS_PINBALL || (loss_param > 0.0 && loss_param < 1.0),
                "loss_param (the tau of the pinball loss) must lie in (0, 1), but got ", loss_param);
    const float *w = weight_row(weights, data_points, d);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size}, at::kFloat, d.dev), grad = empty({pop_size, gp_len}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_weighted_gradient((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, d.value,
                                            d.type, d.size, d.X, d.y, w, (int)loss_kind, loss_param, loss.data_ptr<float>(), grad.data_ptr<float>(),
                                            current_stream(d.dev)),
             "tree_SR_weighted_gradient");
    return {loss, grad};
}

// loss and normal equations of the weighted MSE (evogp_hip_sr_weighted_normal_eq)
std::tuple<Tensor, Tensor> tree_SR_weighted_normal_eq(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                                      const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                      const Tensor &labels, const c10::optional<Tensor> &weights) {
    const Dataset d = check_dataset("tree_SR_weighted_normal_eq", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    const float *w = weight_row(weights, data_points, d);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size}, at::kFloat, d.dev), normal = empty({pop_size, (int64_t)EVOGP_LM_NORMAL_WORDS}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_weighted_normal_eq((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, d.value,
                                             d.type, d.size, d.X, d.y, w, loss.data_ptr<float>(), normal.data_ptr<float>(), current_stream(d.dev)),
             "tree_SR_weighted_normal_eq");
    return {loss, normal};
}

// multi-gene fitness (evogp_hip_sr_gene_fitness): loss (pop,), coef (pop, 1 + out_len) = intercept, weights; with_moments: also the
// (pop, out_len (out_len + 5) / 2) float64 moments the solve read
Tensor3 gene_fitness_impl(const char *op, bool with_moments, int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                          const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels) {
    const Dataset d = check_dataset(op, OutLen::Genes, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size}, at::kFloat, d.dev), coef = empty({pop_size, 1 + out_len}, at::kFloat, d.dev), moments;
    if (with_moments) moments = empty({pop_size, out_len * (out_len + 5) / 2}, at::kDouble, d.dev);
    check_rc(evogp_hip_sr_gene_fitness((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, d.value,
                                       d.type, d.size, d.X, d.y, loss.data_ptr<float>(), coef.data_ptr<float>(),
                                       with_moments ? moments.data_ptr<double>() : nullptr, current_stream(d.dev)),
             op);
    return {loss, coef, moments};
}

std::tuple<Tensor, Tensor> tree_SR_gene_fitness(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                                const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                const Tensor &labels) {
    const Tensor3 r = gene_fitness_impl("tree_SR_gene_fitness", false, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    return {std::get<0>(r), std::get<1>(r)};
}

Tensor3 tree_SR_gene_moments(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                             const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels) {
    return gene_fitness_impl("tree_SR_gene_moments", true, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
}

// every row T as ADD(MUL(T, slope), intercept) in rows of out_gp_len words (evogp_hip_wrap_linear); applied (pop,) uint8
Tensor4 tree_wrap_linear(int64_t out_gp_len, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &coef) {
    const Forest f = Forest::infer(value, type, size);
    TORCH_CHECK(out_gp_len >= f.gp_len && out_gp_len <= kMaxStack, "out_gp_len must be in range [", f.gp_len, ", ", kMaxStack, "], but got ", out_gp_len);
    check_tensor(coef, {f.pop, 2}, "coef", f.dev, at::kFloat);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(f.pop, out_gp_len, f.dev);
    Tensor applied = empty({f.pop}, at::kByte, f.dev);
    check_rc(evogp_hip_wrap_linear((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)out_gp_len, f.value, f.type, f.size, coef.data_ptr<float>(), out.value,
                                   out.type, out.size, applied.data_ptr<uint8_t>(), current_stream(f.dev)),
             "tree_wrap_linear");
    return out.with(applied);
}

// hoist the best subtree, fold the row-constant ones (evogp_hip_prune_rows): a new forest, the chosen roots and their losses
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> tree_prune(int64_t out_len, bool hoist, bool fold, const Tensor &value, const Tensor &type,
                                                              const Tensor &size, const Tensor &node_err, const Tensor &node_const) {
    TORCH_CHECK(out_len == 1, "tree_prune: single-output trees only (out_len must be 1), but got ", out_len);
    const Forest f = Forest::infer(value, type, size);
    check_tensor(node_err, {f.pop, f.gp_len}, "node_err", f.dev, at::kFloat);
    check_tensor(node_const, {f.pop, f.gp_len}, "node_const", f.dev, at::kFloat);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(f.pop, f.gp_len, f.dev);
    Tensor root_pos = empty({f.pop}, at::kInt, f.dev), loss = empty({f.pop}, at::kFloat, f.dev);
    check_rc(evogp_hip_prune_rows((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)out_len, hoist ? 1 : 0, fold ? 1 : 0, f.value, f.type, f.size,
                                  node_err.data_ptr<float>(), node_const.data_ptr<float>(), out.value, out.type, out.size, root_pos.data_ptr<int>(),
                                  loss.data_ptr<float>(), current_stream(f.dev)),
             "tree_prune");
    return {out.tv, out.tt, out.ts, root_pos, loss};
}

// one iteration of the constant descent, in place (include/evogp_hip.h evogp_hip_sr_const_step); phase 2 ignores loss_cand / grad_cand
void tree_SR_const_step(int64_t phase, int64_t out_len, Tensor value, const Tensor &type, const Tensor &size, Tensor value_cand, Tensor loss,
                        Tensor grad, const Tensor &loss_cand, const Tensor &grad_cand, Tensor step) {
    TORCH_CHECK(phase >= 1 && phase <= 3, "phase must be 1, 2 or 3, but got ", phase);
    TORCH_CHECK(out_len > 0, "out_len must be larger than 0, but got ", out_len);
    const Forest f = Forest::infer(value, type, size);
    check_tensor(value_cand, {f.pop, f.gp_len}, "value_cand", f.dev, at::kFloat);
    check_tensor(loss, {f.pop}, "loss", f.dev, at::kFloat);
    check_tensor(grad, {f.pop, f.gp_len}, "grad", f.dev, at::kFloat);
    check_tensor(step, {f.pop}, "step", f.dev, at::kFloat);
    if (phase & 1) {
        check_tensor(loss_cand, {f.pop}, "loss_cand", f.dev, at::kFloat);
        check_tensor(grad_cand, {f.pop, f.gp_len}, "grad_cand", f.dev, at::kFloat);
    }
    c10::DeviceGuard guard(f.dev);
    check_rc(evogp_hip_sr_const_step((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)out_len, (int)phase, f.value, f.type, f.size,
                                     value_cand.data_ptr<float>(), loss.data_ptr<float>(), grad.data_ptr<float>(),
                                     (phase & 1) ? loss_cand.data_ptr<float>() : nullptr, (phase & 1) ? grad_cand.data_ptr<float>() : nullptr,
                                     step.data_ptr<float>(), current_stream(f.dev)),
             "tree_SR_const_step");
}

// loss and Gauss-Newton normal equations of every single-output tree (include/evogp_hip.h evogp_hip_sr_normal_eq)
std::tuple<Tensor, Tensor> tree_SR_normal_eq(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                                             const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                             const Tensor &labels) {
    const Dataset d = check_dataset("tree_SR_normal_eq", OutLen::One, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    c10::DeviceGuard guard(d.dev);
    Tensor loss = empty({pop_size}, at::kFloat, d.dev), normal = empty({pop_size, (int64_t)EVOGP_LM_NORMAL_WORDS}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_normal_eq((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, d.value, d.type,
                                    d.size, d.X, d.y, loss.data_ptr<float>(), normal.data_ptr<float>(), current_stream(d.dev)),
             "tree_SR_normal_eq");
    return {loss, normal};
}

// one Levenberg-Marquardt iteration on the constants, in place (include/evogp_hip.h evogp_hip_sr_lm_step); phase 2 ignores loss_cand / normal_cand
void tree_SR_lm_step(int64_t phase, Tensor value, const Tensor &type, const Tensor &size, Tensor value_cand, Tensor loss, Tensor normal,
                     const Tensor &loss_cand, const Tensor &normal_cand, Tensor damping) {
    TORCH_CHECK(phase >= 1 && phase <= 3, "phase must be 1, 2 or 3, but got ", phase);
    const Forest f = Forest::infer(value, type, size);
    const int64_t words = EVOGP_LM_NORMAL_WORDS;
    check_tensor(value_cand, {f.pop, f.gp_len}, "value_cand", f.dev, at::kFloat);
    check_tensor(loss, {f.pop}, "loss", f.dev, at::kFloat);
    check_tensor(normal, {f.pop, words}, "normal", f.dev, at::kFloat);
    check_tensor(damping, {f.pop}, "damping", f.dev, at::kFloat);
    if (phase & 1) {
        check_tensor(loss_cand, {f.pop}, "loss_cand", f.dev, at::kFloat);
        check_tensor(normal_cand, {f.pop, words}, "normal_cand", f.dev, at::kFloat);
    }
    c10::DeviceGuard guard(f.dev);
    check_rc(evogp_hip_sr_lm_step((unsigned)f.pop, (unsigned)f.gp_len, 1u, (int)phase, f.value, f.type, f.size, value_cand.data_ptr<float>(),
                                  loss.data_ptr<float>(), normal.data_ptr<float>(), (phase & 1) ? loss_cand.data_ptr<float>() : nullptr,
                                  (phase & 1) ? normal_cand.data_ptr<float>() : nullptr, damping.data_ptr<float>(), current_stream(f.dev)),
             "tree_SR_lm_step");
}

// case-major per-case errors (D, pop) of every tree (include/evogp_hip.h evogp_hip_sr_case_errors), validated like tree_batch_evaluate
Tensor tree_SR_case_errors(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, bool use_mse,
                           const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels) {
    const Dataset d = check_dataset("tree_SR_case_errors", OutLen::Any, pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, labels);
    c10::DeviceGuard guard(d.dev);
    Tensor errors = empty({data_points, pop_size}, at::kFloat, d.dev);
    check_rc(evogp_hip_sr_case_errors((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len,
                                      use_mse ? 1 : 0, d.value, d.type, d.size, d.X, d.y, errors.data_ptr<float>(), current_stream(d.dev)),
             "tree_SR_case_errors");
    return errors;
}

// int32[n_events]: the winners of n_events epsilon-lexicase events over case-major errors (n, pop) (evogp_hip_lexicase_select); the
// workspace comes from torch's caching allocator
Tensor lexicase_select(const Tensor &errors, const Tensor &eps, int64_t n_events, int64_t seed, int64_t generation) {
    TORCH_CHECK(errors.is_cuda() && errors.is_contiguous() && errors.scalar_type() == at::kFloat && errors.dim() == 2,
                "errors must be a contiguous float32 CUDA tensor of shape (n_cases, pop)");
    const int64_t n = errors.size(0), pop = errors.size(1);
    TORCH_CHECK(n > 0 && pop > 0 && pop <= 0x7FFFFFFF, "errors must hold at least one case and one tree, got shape ", errors.sizes());
    TORCH_CHECK(n_events >= 0 && n_events <= 0x7FFFFFFF, "n_events must be in [0, 2^31), but got ", n_events);
    const c10::Device dev = errors.device();
    check_tensor(eps, {n}, "eps", dev, at::kFloat);
    c10::DeviceGuard guard(dev);
    Tensor winners = empty({n_events}, at::kInt, dev);
    if (n_events == 0) return winners;
    unsigned long long bytes = 0;
    check_rc(evogp_hip_lexicase_workspace_bytes((unsigned)n, (unsigned)pop, (unsigned)n_events, &bytes), "lexicase_select");
    Tensor ws = empty({(int64_t)bytes}, at::kByte, dev);
    check_rc(evogp_hip_lexicase_select((unsigned)n, (unsigned)pop, errors.data_ptr<float>(), eps.data_ptr<float>(), (unsigned)n_events, seed,
                                       generation, winners.data_ptr<int>(), ws.data_ptr(), current_stream(dev)),
             "lexicase_select");
    return winners;
}

// int64[pop]: the bits of the 64-bit structure hash of every tree (evogp_hip_tree_hash)
Tensor tree_hash(const Tensor &value, const Tensor &type, const Tensor &size) {
    const Forest f = Forest::infer(value, type, size);
    c10::DeviceGuard guard(f.dev);
    Tensor hash = empty({f.pop}, at::kLong, f.dev);
    check_rc(evogp_hip_tree_hash((unsigned)f.pop, (unsigned)f.gp_len, f.value, f.type, f.size, (unsigned long long *)hash.data_ptr<int64_t>(),
                                 current_stream(f.dev)),
             "tree_hash");
    return hash;
}

// the box of the interval ops: lower and upper, (var_len,) float32 each; returns var_len
int64_t check_box(const Tensor &lower, const Tensor &upper, const c10::Device &dev) {
    TORCH_CHECK(lower.dim() == 1 && lower.size(0) > 0, "lower must be a (var_len,) tensor with var_len > 0");
    check_tensor(lower, {lower.size(0)}, "lower", dev, at::kFloat);
    check_tensor(upper, {lower.size(0)}, "upper", dev, at::kFloat);
    return lower.size(0);
}

// (lo float32, hi float32, flags uint8), each (pop, gp_len): the interval of every subtree over the box [lower, upper] (evogp_hip_tree_intervals)
std::tuple<Tensor, Tensor, Tensor> tree_intervals(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &lower,
                                                  const Tensor &upper) {
    const Forest f = Forest::infer(value, type, size);
    const int64_t var_len = check_box(lower, upper, f.dev);
    c10::DeviceGuard guard(f.dev);
    Tensor lo = empty({f.pop, f.gp_len}, at::kFloat, f.dev), hi = empty({f.pop, f.gp_len}, at::kFloat, f.dev);
    Tensor flags = empty({f.pop, f.gp_len}, at::kByte, f.dev);
    check_rc(evogp_hip_tree_intervals((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)var_len, f.value, f.type, f.size, lower.data_ptr<float>(),
                                      upper.data_ptr<float>(), lo.data_ptr<float>(), hi.data_ptr<float>(), flags.data_ptr<uint8_t>(),
                                      current_stream(f.dev)),
             "tree_intervals");
    return {lo, hi, flags};
}

// (vlo, vhi float32, vflags uint8), each (pop, gp_len): enclosures of the real value of every subtree over the box [lower, upper]; (dlo, dhi
// float32, dflags uint8), each (K, pop, gp_len): bounds on its partial derivative in variable wrt[k] (evogp_hip_tree_derivative_intervals)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> tree_derivative_intervals(const Tensor &value, const Tensor &type, const Tensor &size,
                                                                                   const Tensor &lower, const Tensor &upper, const Tensor &wrt) {
    const Forest f = Forest::infer(value, type, size);
    const int64_t var_len = check_box(lower, upper, f.dev);
    TORCH_CHECK(wrt.dim() == 1 && wrt.size(0) > 0 && wrt.size(0) <= 65535, "wrt must be a (K,) tensor with 1 <= K <= 65535");
    const int64_t K = wrt.size(0);
    check_tensor(wrt, {K}, "wrt", f.dev, at::kInt);
    c10::DeviceGuard guard(f.dev);
    Tensor vlo = empty({f.pop, f.gp_len}, at::kFloat, f.dev), vhi = empty({f.pop, f.gp_len}, at::kFloat, f.dev);
    Tensor vflags = empty({f.pop, f.gp_len}, at::kByte, f.dev);
    Tensor dlo = empty({K, f.pop, f.gp_len}, at::kFloat, f.dev), dhi = empty({K, f.pop, f.gp_len}, at::kFloat, f.dev);
    Tensor dflags = empty({K, f.pop, f.gp_len}, at::kByte, f.dev);
    check_rc(evogp_hip_tree_derivative_intervals((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)var_len, f.value, f.type, f.size,
                                                 lower.data_ptr<float>(), upper.data_ptr<float>(), (unsigned)K, wrt.data_ptr<int>(),
                                                 vlo.data_ptr<float>(), vhi.data_ptr<float>(), vflags.data_ptr<uint8_t>(), dlo.data_ptr<float>(),
                                                 dhi.data_ptr<float>(), dflags.data_ptr<uint8_t>(), current_stream(f.dev)),
             "tree_derivative_intervals");
    return {vlo, vhi, vflags, dlo, dhi, dflags};
}

// the prologue of the two input-gradient ops: the forest, X (D, var_len) and the requested variables (checked here: the C entry reads
// wrt on the host); returns D and var_len
struct XgradCall {
    Forest f;
    int64_t D, var_len, V;
    int wrt[EVOGP_XGRAD_MAX_VARS];
};

XgradCall check_xgrad(const char *op, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, at::IntArrayRef wrt) {
    XgradCall c{Forest::infer(value, type, size), 0, 0, 0, {}};
    TORCH_CHECK(variables.dim() == 2 && variables.size(0) > 0 && variables.size(1) > 0, op,
                ": variables must be a (data_points, var_len) tensor with data_points > 0 and var_len > 0, but got shape ", variables.sizes());
    TORCH_CHECK(variables.size(0) <= 0x7FFFFFFF, "too many data points: ", variables.size(0));
    c.D = variables.size(0), c.var_len = variables.size(1), c.V = (int64_t)wrt.size();
    check_tensor(variables, {c.D, c.var_len}, "variables", c.f.dev, at::kFloat);
    TORCH_CHECK(c.V >= 1 && c.V <= EVOGP_XGRAD_MAX_VARS, op, ": wrt must hold 1 to ", EVOGP_XGRAD_MAX_VARS, " variables, but got ", c.V);
    for (int64_t k = 0; k < c.V; ++k) {
        TORCH_CHECK(wrt[k] >= 0 && wrt[k] < c.var_len, op, ": wrt[", k, "] must be in range [0, ", c.var_len, "), but got ", wrt[k]);
        for (int64_t j = 0; j < k; ++j) TORCH_CHECK(wrt[j] != wrt[k], op, ": wrt holds variable ", wrt[k], " twice");
        c.wrt[k] = (int)wrt[k];
    }
    return c;
}

// (pred (pop, D), dpred (V, pop, D)) float32: the prediction and its partial derivatives in the variables wrt on every data row
// (evogp_hip_sr_input_gradient)
std::tuple<Tensor, Tensor> tree_SR_input_gradient(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                  at::IntArrayRef wrt) {
    const XgradCall c = check_xgrad("tree_SR_input_gradient", value, type, size, variables, wrt);
    c10::DeviceGuard guard(c.f.dev);
    Tensor pred = empty({c.f.pop, c.D}, at::kFloat, c.f.dev), dpred = empty({c.V, c.f.pop, c.D}, at::kFloat, c.f.dev);
    check_rc(evogp_hip_sr_input_gradient((unsigned)c.f.pop, (unsigned)c.D, (unsigned)c.f.gp_len, (unsigned)c.var_len, 1u, c.f.value, c.f.type,
                                         c.f.size, variables.data_ptr<float>(), (unsigned)c.V, c.wrt, pred.data_ptr<float>(),
                                         dpred.data_ptr<float>(), current_stream(c.f.dev)),
             "tree_SR_input_gradient");
    return {pred, dpred};
}

// (loss (pop, 1 + V) float32, violations (pop, V) int32): the squared error of the prediction and of every requested derivative against
// dlabels (D, V) (None: zeros), and the rows whose derivative leaves [dmin, dmax] ((V,) each; None: unbounded) (evogp_hip_sr_derivative_loss)
std::tuple<Tensor, Tensor> tree_SR_derivative_loss(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                   const Tensor &labels, const c10::optional<Tensor> &dlabels, at::IntArrayRef wrt,
                                                   const c10::optional<Tensor> &dmin, const c10::optional<Tensor> &dmax) {
    const XgradCall c = check_xgrad("tree_SR_derivative_loss", value, type, size, variables, wrt);
    check_tensor(labels, {c.D, 1}, "labels", c.f.dev, at::kFloat);
    if (dlabels.has_value()) check_tensor(*dlabels, {c.D, c.V}, "dlabels", c.f.dev, at::kFloat);
    if (dmin.has_value()) check_tensor(*dmin, {c.V}, "dmin", c.f.dev, at::kFloat);
    if (dmax.has_value()) check_tensor(*dmax, {c.V}, "dmax", c.f.dev, at::kFloat);
    c10::DeviceGuard guard(c.f.dev);
    Tensor loss = empty({c.f.pop, 1 + c.V}, at::kFloat, c.f.dev), viol = empty({c.f.pop, c.V}, at::kInt, c.f.dev);
    check_rc(evogp_hip_sr_derivative_loss((unsigned)c.f.pop, (unsigned)c.D, (unsigned)c.f.gp_len, (unsigned)c.var_len, 1u, c.f.value, c.f.type,
                                          c.f.size, variables.data_ptr<float>(), labels.data_ptr<float>(),
                                          dlabels.has_value() ? dlabels->data_ptr<float>() : nullptr, (unsigned)c.V, c.wrt,
                                          dmin.has_value() ? dmin->data_ptr<float>() : nullptr, dmax.has_value() ? dmax->data_ptr<float>() : nullptr,
                                          loss.data_ptr<float>(), viol.data_ptr<int>(), current_stream(c.f.dev)),
             "tree_SR_derivative_loss");
    return {loss, viol};
}

// the prologue of the two semantic-backpropagation ops: the forest, X (D, var_len), y (D,) or (D, 1), pos (pop,) int32
struct BackpropCall {
    Forest f;
    int64_t D, var_len;
};

// (labels == nullptr: the midpoint ops, which take their target from a mate)
BackpropCall check_backprop(const char *op, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                            const Tensor *labels, const Tensor &pos) {
    BackpropCall c{Forest::infer(value, type, size), 0, 0};
    TORCH_CHECK(variables.dim() == 2 && variables.size(0) > 0 && variables.size(1) > 0, op,
                ": variables must be a (data_points, var_len) tensor with data_points > 0 and var_len > 0, but got shape ", variables.sizes());
    TORCH_CHECK(variables.size(0) <= 0x7FFFFFFF, "too many data points: ", variables.size(0));
    c.D = variables.size(0), c.var_len = variables.size(1);
    check_tensor(variables, {c.D, c.var_len}, "variables", c.f.dev, at::kFloat);
    if (labels && labels->dim() == 2) check_tensor(*labels, {c.D, 1}, "labels", c.f.dev, at::kFloat);   // (D,) or (D, 1)
    else if (labels) check_tensor(*labels, {c.D}, "labels", c.f.dev, at::kFloat);
    check_tensor(pos, {c.f.pop}, "pos", c.f.dev, at::kInt);
    return c;
}

// (desired float32 (pop, D), state uint8 (pop, D), status int32 (pop,)): the value the subtree at node pos[t] must return on every row for
// the tree to hit the label (evogp_hip_sr_desired)
std::tuple<Tensor, Tensor, Tensor> tree_SR_desired(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables,
                                                   const Tensor &labels, const Tensor &pos) {
    const BackpropCall c = check_backprop("tree_SR_desired", value, type, size, variables, &labels, pos);
    c10::DeviceGuard guard(c.f.dev);
    Tensor desired = empty({c.f.pop, c.D}, at::kFloat, c.f.dev), state = empty({c.f.pop, c.D}, at::kByte, c.f.dev);
    Tensor status = empty({c.f.pop}, at::kInt, c.f.dev);
    check_rc(evogp_hip_sr_desired((unsigned)c.f.pop, (unsigned)c.D, (unsigned)c.f.gp_len, (unsigned)c.var_len, 1u, c.f.value, c.f.type, c.f.size,
                                  variables.data_ptr<float>(), labels.data_ptr<float>(), pos.data_ptr<int>(), desired.data_ptr<float>(),
                                  state.data_ptr<uint8_t>(), status.data_ptr<int>(), current_stream(c.f.dev)),
             "tree_SR_desired");
    return {desired, state, status};
}

// (best int32 (pop,), dist float64 (pop, K), const float32 (pop,), const_dist float64 (pop,), counts int32 (pop, 3), status int32 (pop,)): the
// desired values of tree_SR_desired matched against the library semantics lib (K, D) without a (pop, D) array (evogp_hip_sr_backprop_match).
// The kernel reads the library transposed: the (D, K) copy is made here, once per call
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> tree_SR_backprop_match(const Tensor &value, const Tensor &type, const Tensor &size,
                                                                                const Tensor &variables, const Tensor &labels, const Tensor &pos,
                                                                                const Tensor &lib) {
    const BackpropCall c = check_backprop("tree_SR_backprop_match", value, type, size, variables, &labels, pos);
    TORCH_CHECK(lib.dim() == 2 && lib.size(0) >= 1 && lib.size(0) <= EVOGP_BACKPROP_MAX_LIB,
                "tree_SR_backprop_match: lib must be a (K, data_points) tensor with K in [1, ", EVOGP_BACKPROP_MAX_LIB, "], but got shape ", lib.sizes());
    const int64_t K = lib.size(0);
    check_tensor(lib, {K, c.D}, "lib", c.f.dev, at::kFloat);
    c10::DeviceGuard guard(c.f.dev);
    Tensor lib_t = lib.t().contiguous();
    Tensor best = empty({c.f.pop}, at::kInt, c.f.dev), dist = empty({c.f.pop, K}, at::kDouble, c.f.dev);
    Tensor cnst = empty({c.f.pop}, at::kFloat, c.f.dev), const_dist = empty({c.f.pop}, at::kDouble, c.f.dev);
    Tensor counts = empty({c.f.pop, 3}, at::kInt, c.f.dev), status = empty({c.f.pop}, at::kInt, c.f.dev);
    check_rc(evogp_hip_sr_backprop_match((unsigned)c.f.pop, (unsigned)c.D, (unsigned)c.f.gp_len, (unsigned)c.var_len, 1u, c.f.value, c.f.type,
                                         c.f.size, variables.data_ptr<float>(), labels.data_ptr<float>(), pos.data_ptr<int>(), (unsigned)K,
                                         lib_t.data_ptr<float>(), dist.data_ptr<double>(), best.data_ptr<int>(), cnst.data_ptr<float>(),
                                         const_dist.data_ptr<double>(), counts.data_ptr<int>(), status.data_ptr<int>(), current_stream(c.f.dev)),
             "tree_SR_backprop_match");
    return {best, dist, cnst, const_dist, counts, status};
}

// the mates of the two midpoint ops: a forest of n_mates >= 1 rows of the recipients' width on their device, and mate (pop,) int32 (its
// RANGE is the kernel's to report: status 4)
Forest check_mates(const char *op, const BackpropCall &c, const Tensor &mvalue, const Tensor &mtype, const Tensor &msize, const Tensor &mate) {
    TORCH_CHECK(mvalue.dim() == 2 && mvalue.size(0) >= 1 && mvalue.size(0) <= 0x7FFFFFFF, op,
                ": mate_value must be a (n_mates, gp_len) tensor with n_mates > 0, but got shape ", mvalue.sizes());
    const int64_t n = mvalue.size(0);
    check_tensor(mvalue, {n, c.f.gp_len}, "mate_value", c.f.dev, at::kFloat);
    check_tensor(mtype, {n, c.f.gp_len}, "mate_type", c.f.dev, at::kShort);
    check_tensor(msize, {n, c.f.gp_len}, "mate_size", c.f.dev, at::kShort);
    check_tensor(mate, {c.f.pop}, "mate", c.f.dev, at::kInt);
    Forest m = c.f;
    m.pop = n, m.value = mvalue.data_ptr<float>(), m.type = mtype.data_ptr<int16_t>(), m.size = msize.data_ptr<int16_t>();
    return m;
}

// tree_SR_desired with the root target taken from a mate: 0.5 * T_t + 0.5 * T_mate[t] on every row (evogp_hip_sr_desired_mid); status 4: a
// mate index outside the mates, or a malformed mate
std::tuple<Tensor, Tensor, Tensor> tree_SR_desired_mid(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &mvalue,
                                                       const Tensor &mtype, const Tensor &msize, const Tensor &variables, const Tensor &pos,
                                                       const Tensor &mate) {
    const BackpropCall c = check_backprop("tree_SR_desired_mid", value, type, size, variables, nullptr, pos);
    const Forest m = check_mates("tree_SR_desired_mid", c, mvalue, mtype, msize, mate);
    c10::DeviceGuard guard(c.f.dev);
    Tensor desired = empty({c.f.pop, c.D}, at::kFloat, c.f.dev), state = empty({c.f.pop, c.D}, at::kByte, c.f.dev);
    Tensor status = empty({c.f.pop}, at::kInt, c.f.dev);
    check_rc(evogp_hip_sr_desired_mid((unsigned)c.f.pop, (unsigned)c.D, (unsigned)c.f.gp_len, (unsigned)c.var_len, 1u, c.f.value, c.f.type,
                                      c.f.size, variables.data_ptr<float>(), (unsigned)m.pop, m.value, m.type, m.size, mate.data_ptr<int>(),
                                      pos.data_ptr<int>(), desired.data_ptr<float>(), state.data_ptr<uint8_t>(), status.data_ptr<int>(),
                                      current_stream(c.f.dev)),
             "tree_SR_desired_mid");
    return {desired, state, status};
}

// tree_SR_backprop_match with the root target taken from a mate (evogp_hip_sr_agx_match)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> tree_SR_agx_match(const Tensor &value, const Tensor &type, const Tensor &size,
                                                                           const Tensor &mvalue, const Tensor &mtype, const Tensor &msize,
                                                                           const Tensor &variables, const Tensor &pos, const Tensor &mate,
                                                                           const Tensor &lib) {
    const BackpropCall c = check_backprop("tree_SR_agx_match", value, type, size, variables, nullptr, pos);
    const Forest m = check_mates("tree_SR_agx_match", c, mvalue, mtype, msize, mate);
    TORCH_CHECK(lib.dim() == 2 && lib.size(0) >= 1 && lib.size(0) <= EVOGP_BACKPROP_MAX_LIB,
                "tree_SR_agx_match: lib must be a (K, data_points) tensor with K in [1, ", EVOGP_BACKPROP_MAX_LIB, "], but got shape ", lib.sizes());
    const int64_t K = lib.size(0);
    check_tensor(lib, {K, c.D}, "lib", c.f.dev, at::kFloat);
    c10::DeviceGuard guard(c.f.dev);
    Tensor lib_t = lib.t().contiguous();
    Tensor best = empty({c.f.pop}, at::kInt, c.f.dev), dist = empty({c.f.pop, K}, at::kDouble, c.f.dev);
    Tensor cnst = empty({c.f.pop}, at::kFloat, c.f.dev), const_dist = empty({c.f.pop}, at::kDouble, c.f.dev);
    Tensor counts = empty({c.f.pop, 3}, at::kInt, c.f.dev), status = empty({c.f.pop}, at::kInt, c.f.dev);
    check_rc(evogp_hip_sr_agx_match((unsigned)c.f.pop, (unsigned)c.D, (unsigned)c.f.gp_len, (unsigned)c.var_len, 1u, c.f.value, c.f.type, c.f.size,
                                    variables.data_ptr<float>(), (unsigned)m.pop, m.value, m.type, m.size, mate.data_ptr<int>(),
                                    pos.data_ptr<int>(), (unsigned)K, lib_t.data_ptr<float>(), dist.data_ptr<double>(), best.data_ptr<int>(),
                                    cnst.data_ptr<float>(), const_dist.data_ptr<double>(), counts.data_ptr<int>(), status.data_ptr<int>(),
                                    current_stream(c.f.dev)),
             "tree_SR_agx_match");
    return {best, dist, cnst, const_dist, counts, status};
}

// (units int32 (pop, gp_len, n_dims), flags uint8 (pop, gp_len), violations int32 (pop,)): the unit of every subtree, the variables carrying
// var_units (var_len, n_dims) and, with check_root, the root held to label_units (n_dims,) (evogp_hip_tree_dimensions)
std::tuple<Tensor, Tensor, Tensor> tree_dimensions(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &var_units,
                                                   const Tensor &label_units, bool check_root) {
    const Forest f = Forest::infer(value, type, size);
    TORCH_CHECK(var_units.dim() == 2 && var_units.size(0) > 0 && var_units.size(1) >= 1 && var_units.size(1) <= EVOGP_DIM_MAX_DIMS,
                "var_units must be a (var_len, n_dims) tensor with var_len > 0 and 1 <= n_dims <= ", EVOGP_DIM_MAX_DIMS, ", but got shape ",
                var_units.sizes());
    const int64_t var_len = var_units.size(0), K = var_units.size(1);
    check_tensor(var_units, {var_len, K}, "var_units", f.dev, at::kInt);
    check_tensor(label_units, {K}, "label_units", f.dev, at::kInt);
    c10::DeviceGuard guard(f.dev);
    Tensor units = empty({f.pop, f.gp_len, K}, at::kInt, f.dev), flags = empty({f.pop, f.gp_len}, at::kByte, f.dev);
    Tensor violations = empty({f.pop}, at::kInt, f.dev);
    check_rc(evogp_hip_tree_dimensions((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)var_len, (unsigned)K, f.value, f.type, f.size,
                                       var_units.data_ptr<int>(), label_units.data_ptr<int>(), check_root ? 1 : 0, units.data_ptr<int>(),
                                       flags.data_ptr<uint8_t>(), violations.data_ptr<int>(), current_stream(f.dev)),
             "tree_dimensions");
    return {units, flags, violations};
}

// (complexity int32, height int16, depth int16, each (pop, gp_len); nest uint8 (pop, gp_len, R); flags uint8 (pop, gp_len); violations
// int32 (pop,)): the structural pass under cost (32,), operand_limit (32, 3) and R <= 8 nesting rules (rule_outer, rule_inner, rule_limit,
// (R,) each; R == 0: empty tensors); max_depth, max_complexity: -1 for none (evogp_hip_tree_structure)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> tree_structure(const Tensor &value, const Tensor &type, const Tensor &size,
                                                                        const Tensor &cost, const Tensor &operand_limit,
                                                                        const Tensor &rule_outer, const Tensor &rule_inner,
                                                                        const Tensor &rule_limit, int64_t max_depth, int64_t max_complexity) {
    const Forest f = Forest::infer(value, type, size);
    check_tensor(cost, {EVOGP_STRUCT_SYMBOLS}, "cost", f.dev, at::kInt);
    check_tensor(operand_limit, {EVOGP_STRUCT_SYMBOLS, 3}, "operand_limit", f.dev, at::kInt);
    TORCH_CHECK(rule_outer.dim() == 1 && rule_outer.size(0) <= EVOGP_STRUCT_MAX_RULES, "rule_outer must be a (R,) tensor with 0 <= R <= ",
                EVOGP_STRUCT_MAX_RULES, ", but got shape ", rule_outer.sizes());
    const int64_t R = rule_outer.size(0);
    check_tensor(rule_outer, {R}, "rule_outer", f.dev, at::kInt);
    check_tensor(rule_inner, {R}, "rule_inner", f.dev, at::kInt);
    check_tensor(rule_limit, {R}, "rule_limit", f.dev, at::kInt);
    TORCH_CHECK(max_depth >= -1 && max_depth <= 0x7FFFFFFF, "max_depth must be -1 (none) or >= 0, but got ", max_depth);
    TORCH_CHECK(max_complexity >= -1 && max_complexity <= 0x7FFFFFFF, "max_complexity must be -1 (none) or >= 0, but got ", max_complexity);
    c10::DeviceGuard guard(f.dev);
    Tensor complexity = empty({f.pop, f.gp_len}, at::kInt, f.dev), height = empty({f.pop, f.gp_len}, at::kShort, f.dev);
    Tensor depth = empty({f.pop, f.gp_len}, at::kShort, f.dev), nest = empty({f.pop, f.gp_len, R}, at::kByte, f.dev);
    Tensor flags = empty({f.pop, f.gp_len}, at::kByte, f.dev), violations = empty({f.pop}, at::kInt, f.dev);
    check_rc(evogp_hip_tree_structure((unsigned)f.pop, (unsigned)f.gp_len, (unsigned)R, f.value, f.type, f.size, cost.data_ptr<int>(),
                                      operand_limit.data_ptr<int>(), R ? rule_outer.data_ptr<int>() : nullptr,
                                      R ? rule_inner.data_ptr<int>() : nullptr, R ? rule_limit.data_ptr<int>() : nullptr, (int)max_depth,
                                      (int)max_complexity, complexity.data_ptr<int>(), height.data_ptr<int16_t>(), depth.data_ptr<int16_t>(),
                                      R ? nest.data_ptr<uint8_t>() : nullptr, flags.data_ptr<uint8_t>(), violations.data_ptr<int>(),
                                      current_stream(f.dev)),
             "tree_structure");
    return {complexity, height, depth, nest, flags, violations};
}

// int32[pop]: the smallest tree index whose row equals row t (evogp_hip_tree_classes); `hash` decides which rows are compared; the
// workspace comes from torch's caching allocator
Tensor tree_classes(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &hash) {
    const Forest f = Forest::infer(value, type, size);
    check_tensor(hash, {f.pop}, "hash", f.dev, at::kLong);
    c10::DeviceGuard guard(f.dev);
    Tensor class_id = empty({f.pop}, at::kInt, f.dev);
    unsigned long long bytes = 0;
    check_rc(evogp_hip_tree_classes_workspace_bytes((unsigned)f.pop, &bytes), "tree_classes");
    Tensor ws = empty({(int64_t)bytes}, at::kByte, f.dev);
    check_rc(evogp_hip_tree_classes((unsigned)f.pop, (unsigned)f.gp_len, f.value, f.type, f.size, (const unsigned long long *)hash.data_ptr<int64_t>(),
                                    class_id.data_ptr<int>(), ws.data_ptr(), current_stream(f.dev)),
             "tree_classes");
    return class_id;
}

// the prologue of the semantic ops: a single-output forest and the rows of a dataset, no labels; returns variables' pointer
const float *check_semantic(const char *op, const Forest &f, int64_t data_points, int64_t var_len, int64_t out_len, const Tensor &variables) {
    TORCH_CHECK(var_len > 0, "var_len must be larger than 0, but got ", var_len);
    TORCH_CHECK(out_len == 1, op, ": single-output trees only (out_len must be 1), but got ", out_len);
    TORCH_CHECK(data_points > 0, "data_points must be larger than 0, but got ", data_points);
    TORCH_CHECK(f.pop <= 0x7FFFFFFF && data_points <= 0x7FFFFFFF, "pop_size and data_points must be below 2^31, but got ", f.pop, " and ", data_points);
    check_tensor(variables, {data_points, var_len}, "variables", f.dev, at::kFloat);
    return variables.data_ptr<float>();
}

// int64[pop]: the bits of the 64-bit signature of every tree's predictions on the rows of `variables` (evogp_hip_sr_semantic_hash);
// the workspace comes from torch's caching allocator
Tensor tree_SR_semantic_hash(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                             const Tensor &type, const Tensor &size, const Tensor &variables) {
    const Forest f(pop_size, gp_len, value, type, size);
    const float *X = check_semantic("tree_SR_semantic_hash", f, data_points, var_len, out_len, variables);
    c10::DeviceGuard guard(f.dev);
    Tensor sig = empty({pop_size}, at::kLong, f.dev);
    unsigned long long bytes = 0;
    check_rc(evogp_hip_sr_semantic_hash_workspace_bytes((unsigned)pop_size, &bytes), "tree_SR_semantic_hash");
    Tensor ws = empty({(int64_t)bytes}, at::kByte, f.dev);
    check_rc(evogp_hip_sr_semantic_hash((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value,
                                        f.type, f.size, X, (unsigned long long *)sig.data_ptr<int64_t>(), ws.data_ptr(), current_stream(f.dev)),
             "tree_SR_semantic_hash");
    return sig;
}

// int32[pop]: the smallest index of a tree whose predictions equal those of tree t on every row (evogp_hip_sr_semantic_classes); `hash`
// decides which trees are compared; the workspace comes from torch's caching allocator
Tensor tree_SR_semantic_classes(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                                const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &hash) {
    const Forest f(pop_size, gp_len, value, type, size);
    const float *X = check_semantic("tree_SR_semantic_classes", f, data_points, var_len, out_len, variables);
    check_tensor(hash, {pop_size}, "hash", f.dev, at::kLong);
    c10::DeviceGuard guard(f.dev);
    Tensor class_id = empty({pop_size}, at::kInt, f.dev);
    unsigned long long bytes = 0;
    check_rc(evogp_hip_sr_semantic_classes_workspace_bytes((unsigned)pop_size, &bytes), "tree_SR_semantic_classes");
    Tensor ws = empty({(int64_t)bytes}, at::kByte, f.dev);
    check_rc(evogp_hip_sr_semantic_classes((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len,
                                           f.value, f.type, f.size, X, (const unsigned long long *)hash.data_ptr<int64_t>(),
                                           class_id.data_ptr<int>(), ws.data_ptr(), current_stream(f.dev)),
             "tree_SR_semantic_classes");
    return class_id;
}

// int64[pop][gp_len]: the bits of the signature of every subtree's values on the rows of `variables`, 0 on tails and malformed rows
// (evogp_hip_sr_subtree_signatures)
Tensor tree_SR_subtree_signatures(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                                  const Tensor &type, const Tensor &size, const Tensor &variables) {
    const Forest f(pop_size, gp_len, value, type, size);
    const float *X = check_semantic("tree_SR_subtree_signatures", f, data_points, var_len, out_len, variables);
    c10::DeviceGuard guard(f.dev);
    Tensor sig = empty({pop_size, gp_len}, at::kLong, f.dev);
    check_rc(evogp_hip_sr_subtree_signatures((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len,
                                             f.value, f.type, f.size, X, (unsigned long long *)sig.data_ptr<int64_t>(), current_stream(f.dev)),
             "tree_SR_subtree_signatures");
    return sig;
}

// int16[pop][gp_len]: for every node the descendant that takes its value on every row of `variables`, or the node itself
// (evogp_hip_sr_subtree_introns); sig proposes (tree_SR_subtree_signatures' output, or anything), the tape verifies
Tensor tree_SR_subtree_introns(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                               const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &sig) {
    const Forest f(pop_size, gp_len, value, type, size);
    const float *X = check_semantic("tree_SR_subtree_introns", f, data_points, var_len, out_len, variables);
    check_tensor(sig, {pop_size, gp_len}, "sig", f.dev, at::kLong);
    c10::DeviceGuard guard(f.dev);
    Tensor rep = empty({pop_size, gp_len}, at::kShort, f.dev);
    check_rc(evogp_hip_sr_subtree_introns((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value,
                                          f.type, f.size, X, (const unsigned long long *)sig.data_ptr<int64_t>(), rep.data_ptr<int16_t>(),
                                          current_stream(f.dev)),
             "tree_SR_subtree_introns");
    return rep;
}

// every node replaced by its rep, from the root down (evogp_hip_remove_introns): a new forest and the nodes each tree lost
Tensor4 tree_remove_introns(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &rep) {
    const Forest f = Forest::infer(value, type, size);
    check_tensor(rep, {f.pop, f.gp_len}, "rep", f.dev, at::kShort);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(f.pop, f.gp_len, f.dev);
    Tensor removed = empty({f.pop}, at::kInt, f.dev);
    check_rc(evogp_hip_remove_introns((unsigned)f.pop, (unsigned)f.gp_len, f.value, f.type, f.size, rep.data_ptr<int16_t>(), out.value, out.type,
                                      out.size, removed.data_ptr<int>(), current_stream(f.dev)),
             "tree_remove_introns");
    return out.with(removed);
}

// (own float64 (E,), moments float64 (E, M, 3)): the residual moments of first[e] of forest A against candidates[e, m] of forest B on the
// rows of `variables` (evogp_hip_sr_pair_moments); labels (D,) or None (every label 0); the workspace comes from torch's caching allocator
std::tuple<Tensor, Tensor> tree_SR_pair_moments(const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &mvalue,
                                                const Tensor &mtype, const Tensor &msize, const Tensor &variables,
                                                const c10::optional<Tensor> &labels, const Tensor &first, const Tensor &candidates) {
    const char *op = "tree_SR_pair_moments";
    const Forest a = Forest::infer(value, type, size);
    TORCH_CHECK(mvalue.dim() == 2 && mvalue.size(0) >= 1 && mvalue.size(0) <= 0x7FFFFFFF && mvalue.size(1) >= 1 && mvalue.size(1) <= kMaxStack, op,
                ": mate_value must be a (n_mates, mate_gp_len) tensor with n_mates > 0 and mate_gp_len in (0, ", kMaxStack, "], but got shape ",
                mvalue.sizes());
    const int64_t pop_b = mvalue.size(0), len_b = mvalue.size(1);
    check_tensor(mvalue, {pop_b, len_b}, "mate_value", a.dev, at::kFloat);
    check_tensor(mtype, {pop_b, len_b}, "mate_type", a.dev, at::kShort);
    check_tensor(msize, {pop_b, len_b}, "mate_size", a.dev, at::kShort);
    TORCH_CHECK(variables.dim() == 2 && variables.size(0) > 0 && variables.size(1) > 0, op,
                ": variables must be a (data_points, var_len) tensor with data_points > 0 and var_len > 0, but got shape ", variables.sizes());
    TORCH_CHECK(variables.size(0) <= 0x7FFFFFFF, op, ": variables has too many data points: ", variables.size(0));
    const int64_t D = variables.size(0), var_len = variables.size(1);
    check_tensor(variables, {D, var_len}, "variables", a.dev, at::kFloat);
    if (labels.has_value()) check_tensor(*labels, {D}, "labels", a.dev, at::kFloat);
    TORCH_CHECK(first.dim() == 1 && first.size(0) <= 0x7FFFFFFF, op, ": first must be an (events,) tensor, but got shape ", first.sizes());
    const int64_t E = first.size(0);
    check_tensor(first, {E}, "first", a.dev, at::kInt);
    TORCH_CHECK(candidates.dim() == 2 && candidates.size(1) >= 1 && candidates.size(1) <= EVOGP_PAIR_MAX_CANDIDATES, op,
                ": candidates must be an (events, M) tensor with M in [1, ", EVOGP_PAIR_MAX_CANDIDATES, "], but got shape ", candidates.sizes());
    const int64_t M = candidates.size(1);
    check_tensor(candidates, {E, M}, "candidates", a.dev, at::kInt);
    c10::DeviceGuard guard(a.dev);
    Tensor own = empty({E}, at::kDouble, a.dev), moments = empty({E, M, 3}, at::kDouble, a.dev);
    if (E == 0) return {own, moments};   // nothing to launch
    unsigned long long bytes = 0;
    check_rc(evogp_hip_sr_pair_moments_workspace_bytes((unsigned)E, (unsigned)M, &bytes), op);
    Tensor ws = empty({(int64_t)bytes}, at::kByte, a.dev);
    check_rc(evogp_hip_sr_pair_moments((unsigned)E, (unsigned)M, (unsigned)D, (unsigned)var_len, (unsigned)a.pop, (unsigned)a.gp_len, a.value, a.type,
                                       a.size, (unsigned)pop_b, (unsigned)len_b, mvalue.data_ptr<float>(), mtype.data_ptr<int16_t>(),
                                       msize.data_ptr<int16_t>(), variables.data_ptr<float>(),
                                       labels.has_value() ? labels->data_ptr<float>() : nullptr, first.data_ptr<int>(), candidates.data_ptr<int>(),
                                       own.data_ptr<double>(), moments.data_ptr<double>(), ws.data_ptr(), current_stream(a.dev)),
             op);
    return {own, moments};
}

// (member int32[k], count int32[k], n_classes int32[1]): the k largest classes of equal signature among the eligible nodes, each by its
// (size, flat index)-smallest member (evogp_hip_subtree_library_select); the workspace comes from torch's caching allocator
Tensor3 subtree_library_select(const Tensor &sig, const Tensor &size, int64_t min_size, int64_t max_size, int64_t k) {
    TORCH_CHECK(sig.is_cuda() && sig.is_contiguous() && sig.scalar_type() == at::kLong && sig.dim() == 2 && sig.numel() > 0,
                "sig must be a non-empty contiguous int64 (pop_size, gp_len) CUDA tensor");
    const int64_t pop = sig.size(0), gp_len = sig.size(1);
    check_sizes(pop, gp_len);
    TORCH_CHECK(pop * gp_len <= 0x7FFFFFFF, "sig must hold fewer than 2^31 words, but got shape ", sig.sizes());
    const c10::Device dev = sig.device();
    check_tensor(size, {pop, gp_len}, "size", dev, at::kShort);
    TORCH_CHECK(min_size >= 1, "min_size must be at least 1, but got ", min_size);
    TORCH_CHECK(max_size >= min_size && max_size <= 0x7FFFFFFF, "max_size must be in [min_size, 2^31), but got ", max_size, " with min_size ", min_size);
    TORCH_CHECK(k >= 1 && k <= EVOGP_BACKPROP_MAX_LIB, "k must be in [1, ", EVOGP_BACKPROP_MAX_LIB, "], but got ", k);
    c10::DeviceGuard guard(dev);
    Tensor member = empty({k}, at::kInt, dev), count = empty({k}, at::kInt, dev), n_classes = empty({1}, at::kInt, dev);
    unsigned long long bytes = 0;
    check_rc(evogp_hip_subtree_library_select_workspace_bytes((unsigned)pop, (unsigned)gp_len, &bytes), "subtree_library_select");
    Tensor ws = empty({(int64_t)bytes}, at::kByte, dev);
    check_rc(evogp_hip_subtree_library_select((unsigned)pop, (unsigned)gp_len, (const unsigned long long *)sig.data_ptr<int64_t>(),
                                              size.data_ptr<int16_t>(), (int)min_size, (int)max_size, (int)k, member.data_ptr<int>(),
                                              count.data_ptr<int>(), n_classes.data_ptr<int>(), ws.data_ptr(), current_stream(dev)),
             "subtree_library_select");
    return {member, count, n_classes};
}

// (front int32, crowding float32, order int32) of a population on (err, cx) (evogp_hip_pareto_rank); the workspace comes from torch's
// caching allocator
Tensor3 pareto_rank(const Tensor &err, const Tensor &cx, int64_t cx_bound) {
    TORCH_CHECK(err.is_cuda() && err.is_contiguous() && err.scalar_type() == at::kFloat && err.dim() == 1,
                "err must be a contiguous float32 CUDA vector");
    const int64_t pop = err.size(0);
    TORCH_CHECK(pop > 0 && pop < 0x7FFFFFFF, "err must hold at least one tree, got shape ", err.sizes());
    TORCH_CHECK(cx_bound >= 0 && cx_bound <= 65535, "cx_bound must be in [0, 65535], but got ", cx_bound);
    const c10::Device dev = err.device();
    check_tensor(cx, {pop}, "cx", dev, at::kInt);
    c10::DeviceGuard guard(dev);
    Tensor front = empty({pop}, at::kInt, dev), crowding = empty({pop}, at::kFloat, dev), order = empty({pop}, at::kInt, dev);
    unsigned long long bytes = 0;
    check_rc(evogp_hip_pareto_rank_workspace_bytes((unsigned)pop, &bytes), "pareto_rank");
    Tensor ws = empty({(int64_t)bytes}, at::kByte, dev);
    check_rc(evogp_hip_pareto_rank((unsigned)pop, (unsigned)cx_bound, err.data_ptr<float>(), cx.data_ptr<int>(), front.data_ptr<int>(),
                                   crowding.data_ptr<float>(), order.data_ptr<int>(), ws.data_ptr(), current_stream(dev)),
             "pareto_rank");
    return {front, crowding, order};
}

// int32[n]: the winners of n crowded-comparison tournaments among the first `pool` trees of a pareto_rank order (evogp_hip_nsga2_select)
Tensor nsga2_select(const Tensor &order, int64_t pool, int64_t n, int64_t t_size, int64_t seed, int64_t generation) {
    TORCH_CHECK(order.is_cuda() && order.is_contiguous() && order.scalar_type() == at::kInt && order.dim() == 1 && order.size(0) > 0,
                "order must be a non-empty contiguous int32 CUDA vector");
    const int64_t pop = order.size(0);
    TORCH_CHECK(pop < 0x7FFFFFFF, "order is too long: ", pop);
    TORCH_CHECK(pool >= 1 && pool <= pop, "pool must be in [1, ", pop, "], but got ", pool);
    TORCH_CHECK(t_size >= 1 && t_size <= (1 << 20), "t_size must be in [1, 2^20], but got ", t_size);
    TORCH_CHECK(n >= 0 && n <= 0x7FFFFFFF, "n must be in [0, 2^31), but got ", n);
    const c10::Device dev = order.device();
    c10::DeviceGuard guard(dev);
    Tensor winners = empty({n}, at::kInt, dev);
    if (n == 0) return winners;
    check_rc(evogp_hip_nsga2_select((unsigned)pop, order.data_ptr<int>(), (unsigned)pool, (unsigned)n, (unsigned)t_size, seed, generation,
                                    winners.data_ptr<int>(), current_stream(dev)),
             "nsga2_select");
    return winners;
}

Tensor3 tree_generate_offset(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, int64_t const_samples_len,
                             double out_prob, double const_prob, const Tensor &keys, const Tensor &depth2leaf_probs,
                             const Tensor &roulette_funcs, const Tensor &const_samples, int64_t tree_index_offset) {
    return generate_impl(pop_size, gp_len, var_len, out_len, const_samples_len, out_prob, const_prob, keys, depth2leaf_probs,
                         roulette_funcs, const_samples, tree_index_offset, nullptr, 0);
}

// rows of trees with active_word[n] >= active_below are left uninitialised
Tensor3 tree_generate_masked(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, int64_t const_samples_len,
                             double out_prob, double const_prob, const Tensor &keys, const Tensor &depth2leaf_probs,
                             const Tensor &roulette_funcs, const Tensor &const_samples, int64_t tree_index_offset,
                             const Tensor &active_word, int64_t active_below) {
    return generate_impl(pop_size, gp_len, var_len, out_len, const_samples_len, out_prob, const_prob, keys, depth2leaf_probs,
                         roulette_funcs, const_samples, tree_index_offset, &active_word, active_below);
}

Tensor tree_batch_evaluate(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                           const Tensor &type, const Tensor &size, const Tensor &variables) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(var_len > 0 && out_len > 0 && data_points > 0, "var_len, out_len and data_points must be positive");
    check_tensor(variables, {data_points, var_len}, "variables", f.dev, at::kFloat);
    c10::DeviceGuard guard(f.dev);
    Tensor results = empty({pop_size, data_points, out_len}, at::kFloat, f.dev);
    check_rc(evogp_hip_batch_evaluate((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value,
                                      f.type, f.size, variables.data_ptr<float>(), results.data_ptr<float>(), current_stream(f.dev)),
             "tree_batch_evaluate");
    return results;
}

// counts[t] = #rows whose arg-max output (as torch.argmax(clip(softmax(.))) sees it) equals the int32 label
Tensor tree_batch_argmax_count(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len,
                               const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(data_points > 0 && var_len > 0, "data_points and var_len must be larger than 0");
    TORCH_CHECK(out_len >= 2 && out_len <= 16, "out_len must be in [2, 16], but got ", out_len);
    check_tensor(variables, {data_points, var_len}, "variables", f.dev, at::kFloat);
    check_tensor(labels, {data_points}, "labels", f.dev, at::kInt);
    c10::DeviceGuard guard(f.dev);
    Tensor counts = empty({pop_size}, at::kInt, f.dev);
    check_rc(evogp_hip_batch_argmax_count((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value,
                                          f.type, f.size, variables.data_ptr<float>(), labels.data_ptr<int>(), (unsigned *)counts.data_ptr<int>(),
                                          current_stream(f.dev)),
             "tree_batch_argmax_count");
    return counts;
}

// (hits int32[pop][G][C], predicted int32[pop][G][C], loss float64[pop][G]) of a multi-output forest over up to 8 row splits
// (evogp_hip_batch_class_stats); groups: int32[D] or None (every row in split 0, n_groups = 1)
Tensor3 tree_batch_class_stats(int64_t pop_size, int64_t data_points, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                               const Tensor &type, const Tensor &size, const Tensor &variables, const Tensor &labels,
                               const c10::optional<Tensor> &groups, int64_t n_groups) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(data_points > 0 && var_len > 0, "data_points and var_len must be larger than 0");
    TORCH_CHECK(out_len >= 2 && out_len <= 16, "out_len must be in [2, 16], but got ", out_len);
    TORCH_CHECK(n_groups >= 1 && n_groups <= 8, "n_groups must be in [1, 8], but got ", n_groups);
    check_tensor(variables, {data_points, var_len}, "variables", f.dev, at::kFloat);
    check_tensor(labels, {data_points}, "labels", f.dev, at::kInt);
    const bool split = groups.has_value() && groups->defined();
    if (split) check_tensor(*groups, {data_points}, "groups", f.dev, at::kInt);
    else TORCH_CHECK(n_groups == 1, "n_groups must be 1 without groups, but got ", n_groups);
    c10::DeviceGuard guard(f.dev);
    Tensor hits = empty({pop_size, n_groups, out_len}, at::kInt, f.dev), predicted = empty({pop_size, n_groups, out_len}, at::kInt, f.dev);
    Tensor loss = empty({pop_size, n_groups}, at::kDouble, f.dev);
    check_rc(evogp_hip_batch_class_stats((unsigned)pop_size, (unsigned)data_points, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value,
                                         f.type, f.size, variables.data_ptr<float>(), labels.data_ptr<int>(),
                                         split ? groups->data_ptr<int>() : nullptr, (unsigned)n_groups, hits.data_ptr<int>(),
                                         predicted.data_ptr<int>(), loss.data_ptr<double>(), current_stream(f.dev)),
             "tree_batch_class_stats");
    return {hits, predicted, loss};
}

// the operation lists of a multi-output forest (evaluate_prepared.hip): -> (workspace uint8[bytes], info int32[16]; info[0] = trees
// the lists cannot express, which tree_evaluate_prepared then has to send through the stack interpreter)
std::tuple<Tensor, Tensor> tree_evaluate_prepare(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value,
                                                 const Tensor &type, const Tensor &size) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(var_len > 0 && var_len <= 255, "var_len must be in [1, 255], but got ", var_len);
    TORCH_CHECK(out_len >= 2 && out_len <= 32, "out_len must be in [2, 32], but got ", out_len);
    c10::DeviceGuard guard(f.dev);
    const int64_t bytes = (int64_t)evogp_hip_evaluate_workspace_bytes((unsigned)pop_size, (unsigned)gp_len);
    Tensor ws = empty({bytes}, at::kByte, f.dev);
    check_rc(evogp_hip_evaluate_prepare((unsigned)pop_size, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value, f.type, f.size,
                                        ws.data_ptr(), (size_t)bytes, current_stream(f.dev)),
             "tree_evaluate_prepare");
    Tensor info = ws.narrow(0, bytes - 64, 64).view(at::kInt);
    return {ws, info};
}

Tensor tree_evaluate_prepared(int64_t pop_size, int64_t gp_len, int64_t var_len, int64_t out_len, const Tensor &value, const Tensor &type,
                              const Tensor &size, const Tensor &workspace, bool with_fallback, const Tensor &variables) {
    const Forest f(pop_size, gp_len, value, type, size);
    check_tensor(variables, {pop_size, var_len}, "variables", f.dev, at::kFloat);
    check_tensor(workspace, {(int64_t)evogp_hip_evaluate_workspace_bytes((unsigned)pop_size, (unsigned)gp_len)}, "workspace", f.dev, at::kByte);
    c10::DeviceGuard guard(f.dev);
    Tensor results = empty({pop_size, out_len}, at::kFloat, f.dev);
    check_rc(evogp_hip_evaluate_prepared((unsigned)pop_size, (unsigned)gp_len, (unsigned)var_len, (unsigned)out_len, f.value, f.type, f.size,
                                         workspace.data_ptr(), with_fallback ? 1 : 0, variables.data_ptr<float>(), results.data_ptr<float>(),
                                         current_stream(f.dev)),
             "tree_evaluate_prepared");
    return results;
}

// scores = NaN -> -inf, else -errors (negate) or errors: the sign of SymbolicRegression.evaluate and the NaN scrub of StandardPipeline.step in one launch
Tensor fitness_scores(const Tensor &errors, bool negate) {
    TORCH_CHECK(errors.is_cuda() && errors.scalar_type() == at::kFloat && errors.is_contiguous() && errors.dim() == 1 && errors.numel() > 0,
                "fitness_scores: errors must be a non-empty contiguous float32 CUDA vector");
    const c10::DeviceGuard guard(errors.device());
    Tensor out = at::empty_like(errors);
    check_rc(evogp_hip_fitness_scores((unsigned)errors.numel(), negate ? 1 : 0, errors.data_ptr<float>(), out.data_ptr<float>(), current_stream(errors.device())),
             "fitness_scores");
    return out;
}

// int32[rows][n_cols] whose columns [lo, hi) hold the counter-based random words of (seed, generation) (breed.hip); the other
// columns are uninitialised
Tensor random_words(int64_t seed, int64_t generation, int64_t rows, int64_t n_cols, int64_t lo, int64_t hi, c10::Device device) {
    TORCH_CHECK(device.is_cuda(), "random_words: the native generator runs on the GPU");
    TORCH_CHECK(rows > 0 && n_cols > 0 && lo >= 0 && lo <= hi && hi <= n_cols, "random_words: column range out of the array");
    c10::DeviceGuard guard(device);
    Tensor out = at::empty({rows, n_cols}, at::TensorOptions().dtype(at::kInt).device(device));
    check_rc(evogp_hip_random_words(seed, generation, (int)rows, n_cols, lo, hi, out.data_ptr<int>(), current_stream(out.device())), "random_words");
    return out;
}

// int32[n_keep]: the n_elite best trees, then the other survivors, each group in ascending index (select.hip)
Tensor select_survivors(const Tensor &fitness, int64_t n_elite, int64_t n_keep) {
    TORCH_CHECK(fitness.is_cuda() && fitness.is_contiguous() && fitness.scalar_type() == at::kFloat && fitness.dim() == 1,
                "fitness must be a contiguous float32 CUDA vector");
    const int64_t n = fitness.size(0);
    TORCH_CHECK(n > 0 && n_keep > 0 && n_keep <= n && n_elite >= 0 && n_elite <= n_keep, "need 0 <= n_elite <= n_keep <= n, got ", n_elite, ", ", n_keep, ", ", n);
    const c10::Device dev = fitness.device();
    c10::DeviceGuard guard(dev);
    Tensor order = at::empty({n_keep}, at::TensorOptions().dtype(at::kInt).device(dev));
    const int64_t words = (int64_t)(evogp_hip_select_workspace_bytes() / 4);
    const evogp_stream_t stream = current_stream(dev);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    if (capturing) {   // a replayed graph cannot alternate: a fresh zeroed workspace per captured call
        Tensor ws = at::zeros({words}, at::TensorOptions().dtype(at::kInt).device(dev));
        check_rc(evogp_hip_select((unsigned)n, (unsigned)n_elite, (unsigned)n_keep, fitness.data_ptr<float>(), order.data_ptr<int>(), ws.data_ptr(),
                                  stream), "select_survivors");
        return order;
    }
    // two workspaces per (device, stream): this call's was zeroed by the previous call's kernel on the same stream
    struct Slot { Tensor ws; int parity = 0; };
    static std::mutex mu;
    // (leaked on purpose: a static container of tensors would be destroyed at process teardown, after the caching allocator)
    static auto &slots = *new std::map<std::pair<int, void *>, Slot>();
    std::lock_guard<std::mutex> lock(mu);
    Slot &sl = slots[{(int)dev.index(), (void *)stream}];
    if (!sl.ws.defined()) sl.ws = at::zeros({2 * words}, at::TensorOptions().dtype(at::kInt).device(dev));
    int *base = sl.ws.data_ptr<int>();
    int *mine = base + (int64_t)sl.parity * words, *next = base + (int64_t)(1 - sl.parity) * words;
    const int rc = evogp_hip_select_alternating((unsigned)n, (unsigned)n_elite, (unsigned)n_keep, fitness.data_ptr<float>(), order.data_ptr<int>(), mine,
                                                next, stream);
    if (rc != EVOGP_OK) sl.ws = Tensor();   // the halves' zero / dirty protocol is unknown after a failed launch: a fresh workspace next time
    else sl.parity ^= 1;                    // (only a launch that ran has zeroed `next`)
    check_rc(rc, "select_survivors");
    return order;
}

// int32[n_tournaments]: the winner of every tournament of t_size counter-based contenders (select.hip)
Tensor tournament_select(const Tensor &fitness, int64_t n_tournaments, int64_t t_size, int64_t seed, int64_t generation) {
    TORCH_CHECK(fitness.is_cuda() && fitness.is_contiguous() && fitness.scalar_type() == at::kFloat && fitness.dim() == 1,
                "fitness must be a contiguous float32 CUDA vector");
    TORCH_CHECK(fitness.size(0) > 0 && n_tournaments > 0 && t_size > 0, "need a population, tournaments and contenders");
    const c10::Device dev = fitness.device();
    c10::DeviceGuard guard(dev);
    Tensor winners = at::empty({n_tournaments}, at::TensorOptions().dtype(at::kInt).device(dev));
    check_rc(evogp_hip_tournament_select((unsigned)fitness.size(0), (unsigned)n_tournaments, (unsigned)t_size, seed, generation,
                                         fitness.data_ptr<float>(), winners.data_ptr<int>(), current_stream(dev)), "tournament_select");
    return winners;
}

void check_order(const Tensor &order, int64_t need, const c10::Device &dev) {
    TORCH_CHECK(order.is_cuda() && order.is_contiguous() && order.scalar_type() == at::kInt && order.dim() == 1 && order.size(0) >= need &&
                    order.device() == dev,
                "order must be a contiguous int32 CUDA vector of >= max(n_elite, n_surv) entries on the forest's device");
}

Tensor4 breed_default(int64_t pop_size, int64_t gp_len, int64_t n_elite, int64_t n_surv, const Tensor &value, const Tensor &type,
                      const Tensor &size, const Tensor &order, const Tensor &rnd, int64_t mutate_below, const Tensor &donor_value,
                      const Tensor &donor_type, const Tensor &donor_size, bool want_decisions) {
    const Forest f(pop_size, gp_len, value, type, size);
    TORCH_CHECK(n_elite >= 0 && n_elite <= pop_size, "n_elite must be in [0, pop_size], but got ", n_elite);
    TORCH_CHECK(n_surv > 0 && n_surv <= pop_size, "n_surv must be in (0, pop_size], but got ", n_surv);
    TORCH_CHECK(mutate_below >= 0 && mutate_below < (1LL << 32), "mutate_below must fit in 32 bits");
    const int64_t n_new = pop_size - n_elite;
    check_order(order, std::max(n_elite, n_surv), f.dev);
    check_tensor(rnd, {6, n_new}, "rnd", f.dev, at::kInt);
    const Forest donors = Forest::donors(n_new, gp_len, donor_value, donor_type, donor_size, f.dev);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(pop_size, gp_len, f.dev);
    Tensor dec = empty({want_decisions ? n_new : 0, 6}, at::kInt, f.dev);
    check_rc(evogp_hip_breed_default((int)pop_size, (int)gp_len, (int)n_elite, (int)n_surv, f.value, f.type, f.size, order.data_ptr<int>(),
                                     rnd.data_ptr<int>(), (unsigned)mutate_below, donors.value, donors.type, donors.size, out.value, out.type, out.size,
                                     want_decisions ? dec.data_ptr<int>() : nullptr, current_stream(f.dev)),
             "breed_default");
    return out.with(dec);
}

// The table of the row-range breed ops: value / type / size hold the whole population, or only the trees the selection names (a sharded
// run's survivor table), in rows of gp_len words; [row_begin, row_begin + row_count) are the rows of the next generation to make.
Forest check_breed_rows(int64_t pop_size, int64_t gp_len, const Tensor &value, const Tensor &type, const Tensor &size, int64_t mutate_below,
                        int64_t row_begin, int64_t row_count) {
    check_sizes(pop_size, gp_len);
    TORCH_CHECK(row_begin >= 0 && row_count > 0 && row_begin + row_count <= pop_size, "row range out of the population");
    TORCH_CHECK(mutate_below >= 0 && mutate_below < (1LL << 32), "mutate_below must fit in 32 bits");
    TORCH_CHECK(value.dim() == 2 && value.size(0) > 0, "value must be a (rows, gp_len) tensor");
    return Forest(value.size(0), gp_len, value, type, size);
}

// Rows [row_begin, row_begin + row_count) of the next generation from the survivor order (the donors: Donors above).
Tensor3 breed_default_rows(int64_t pop_size, int64_t gp_len, int64_t n_elite, int64_t n_surv, const Tensor &value, const Tensor &type,
                           const Tensor &size, const Tensor &order, const Tensor &rnd, int64_t mutate_below, const Tensor &donor_value,
                           const Tensor &donor_type, const Tensor &donor_size, int64_t row_begin, int64_t row_count) {
    const Forest f = check_breed_rows(pop_size, gp_len, value, type, size, mutate_below, row_begin, row_count);
    TORCH_CHECK(n_elite >= 0 && n_elite <= pop_size && n_surv > 0 && n_surv <= pop_size, "n_elite / n_surv out of range");
    check_order(order, std::max(n_elite, n_surv), f.dev);
    check_tensor(rnd, {6, pop_size - n_elite}, "rnd", f.dev, at::kInt);
    const Donors donors(donor_value, donor_type, donor_size, row_begin, row_count, n_elite, gp_len, f.dev);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(row_count, gp_len, f.dev);
    check_rc(evogp_hip_breed_default_table((int)pop_size, (int)f.pop, (int)gp_len, (int)n_elite, (int)n_surv, f.value, f.type, f.size,
                                           order.data_ptr<int>(), rnd.data_ptr<int>(), (unsigned)mutate_below, donors.value, donors.type, donors.size,
                                           out.value, out.type, out.size, nullptr, (int)row_begin, (int)row_count, current_stream(f.dev)),
             "breed_default_rows");
    return out.tuple();
}

// The same rows for ANY selection operator: the elites and the parents are two lists of table rows (parents may repeat, as
// the survivor indices of a tournament selection do); n_elite / n_surv are the lists' lengths.
Tensor3 breed_rows_impl(int64_t pop_size, int64_t gp_len, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &elite_rows,
                        const Tensor &parent_rows, const Tensor *rnd_or_null, int64_t seed, int64_t generation, int64_t mutate_below,
                        const Tensor &donor_value, const Tensor &donor_type, const Tensor &donor_size, int64_t row_begin, int64_t row_count) {
    const Forest f = check_breed_rows(pop_size, gp_len, value, type, size, mutate_below, row_begin, row_count);
    TORCH_CHECK(elite_rows.dim() == 1 && parent_rows.dim() == 1, "elite_rows / parent_rows must be vectors");
    const int64_t n_elite = elite_rows.size(0), n_surv = parent_rows.size(0);
    TORCH_CHECK(n_elite <= pop_size && n_surv > 0, "need n_elite <= pop_size and at least one parent, got ", n_elite, ", ", n_surv);
    check_order(parent_rows, n_surv, f.dev);
    if (n_elite > 0) check_order(elite_rows, n_elite, f.dev);
    if (rnd_or_null) check_tensor(*rnd_or_null, {6, pop_size - n_elite}, "rnd", f.dev, at::kInt);
    const Donors donors(donor_value, donor_type, donor_size, row_begin, row_count, n_elite, gp_len, f.dev);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(row_count, gp_len, f.dev);
    const int *elites = n_elite > 0 ? elite_rows.data_ptr<int>() : nullptr, *parents = parent_rows.data_ptr<int>();
    const int rc = rnd_or_null
        ? evogp_hip_breed_lists((int)pop_size, (int)f.pop, (int)gp_len, (int)n_elite, (int)n_surv, f.value, f.type, f.size, elites, parents,
                                rnd_or_null->data_ptr<int>(), (unsigned)mutate_below, donors.value, donors.type, donors.size, out.value, out.type,
                                out.size, nullptr, (int)row_begin, (int)row_count, current_stream(f.dev))
        : evogp_hip_breed_lists_hashed((int)pop_size, (int)f.pop, (int)gp_len, (int)n_elite, (int)n_surv, f.value, f.type, f.size, elites, parents, seed,
                                       generation, (unsigned)mutate_below, donors.value, donors.type, donors.size, out.value, out.type, out.size,
                                       nullptr, (int)row_begin, (int)row_count, current_stream(f.dev));
    check_rc(rc, "breed_rows");
    return out.tuple();
}

Tensor3 breed_rows(int64_t pop_size, int64_t gp_len, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &elite_rows,
                   const Tensor &parent_rows, const Tensor &rnd, int64_t mutate_below, const Tensor &donor_value, const Tensor &donor_type,
                   const Tensor &donor_size, int64_t row_begin, int64_t row_count) {
    return breed_rows_impl(pop_size, gp_len, value, type, size, elite_rows, parent_rows, &rnd, 0, 0, mutate_below, donor_value, donor_type, donor_size,
                           row_begin, row_count);
}

// breed_rows with the six words of every offspring computed in the kernel from (seed, generation) instead of read from `rnd`
Tensor3 breed_rows_hashed(int64_t pop_size, int64_t gp_len, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &elite_rows,
                          const Tensor &parent_rows, int64_t seed, int64_t generation, int64_t mutate_below, const Tensor &donor_value,
                          const Tensor &donor_type, const Tensor &donor_size, int64_t row_begin, int64_t row_count) {
    return breed_rows_impl(pop_size, gp_len, value, type, size, elite_rows, parent_rows, nullptr, seed, generation, mutate_below, donor_value,
                           donor_type, donor_size, row_begin, row_count);
}

// the (pop, 2) decisions of the native mutations, or an empty tensor
Tensor decisions(bool want, int64_t pop, const c10::Device &dev) { return want ? empty({pop, 2}, at::kInt, dev) : empty({0}, at::kInt, dev); }

// DeleteMutation (mode 0) / HoistMutation (mode 1) drawn and applied in one launch (include/evogp_hip.h evogp_hip_structural_mutate)
Tensor4 structural_mutate(int64_t mode, double rate, int64_t max_size, bool inner_is_offset, int64_t skip_rows, int64_t seed, int64_t call,
                          const Tensor &value, const Tensor &type, const Tensor &size, bool want_decisions) {
    const Forest f = Forest::infer(value, type, size);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(f.pop, f.gp_len, f.dev);
    Tensor dec = decisions(want_decisions, f.pop, f.dev);
    check_rc(evogp_hip_structural_mutate((int)f.pop, (int)f.gp_len, (int)mode, (float)rate, (int)max_size, inner_is_offset ? 1 : 0, (int)skip_rows, seed,
                                         call, f.value, f.type, f.size, out.value, out.type, out.size, want_decisions ? dec.data_ptr<int>() : nullptr,
                                         current_stream(f.dev)),
             "structural_mutate");
    return out.with(dec);
}

// InsertMutation drawn and applied in one launch over fresh trees from tree_generate_masked_hashed(seed, call, mutate_below) (evogp_hip_insert_mutate)
Tensor4 insert_mutate(int64_t mutate_below, int64_t skip_rows, int64_t seed, int64_t call, const Tensor &value, const Tensor &type,
                      const Tensor &size, const Tensor &donor_value, const Tensor &donor_type, const Tensor &donor_size, bool want_decisions) {
    const Forest f = Forest::infer(value, type, size);
    TORCH_CHECK(mutate_below >= 0 && mutate_below < (1LL << 32), "mutate_below must fit in 32 bits");
    const Forest donors = Forest::donors(f.pop, f.gp_len, donor_value, donor_type, donor_size, f.dev);
    c10::DeviceGuard guard(f.dev);
    const ForestOut out(f.pop, f.gp_len, f.dev);
    Tensor dec = decisions(want_decisions, f.pop, f.dev);
    check_rc(evogp_hip_insert_mutate((int)f.pop, (int)f.gp_len, (unsigned)mutate_below, (int)skip_rows, seed, call, f.value, f.type, f.size, donors.value,
                                     donors.type, donors.size, out.value, out.type, out.size, want_decisions ? dec.data_ptr<int>() : nullptr,
                                     current_stream(f.dev)),
             "insert_mutate");
    return out.with(dec);
}

// Multi / Single Point / Const mutation drawn and applied in one launch: the new value array (evogp_hip_point_mutate)
Tensor point_mutate(int64_t mode, double rate, double intensity, bool per_node, bool modify_output, bool fix_roulette, int64_t skip_rows, int64_t input_len,
                    int64_t output_len, int64_t seed, int64_t call, const Tensor &value, const Tensor &type, const Tensor &size, const Tensor &roulette_ufuncs,
                    const Tensor &roulette_bfuncs, const Tensor &roulette_tfuncs, const Tensor &const_samples) {
    const Forest f = Forest::infer(value, type, size);
    check_tensor(roulette_ufuncs, {29}, "roulette_ufuncs", f.dev, at::kFloat);
    check_tensor(roulette_bfuncs, {29}, "roulette_bfuncs", f.dev, at::kFloat);
    check_tensor(roulette_tfuncs, {29}, "roulette_tfuncs", f.dev, at::kFloat);
    TORCH_CHECK(const_samples.dim() == 1 && const_samples.size(0) > 0, "const_samples must be a non-empty vector");
    check_tensor(const_samples, {const_samples.size(0)}, "const_samples", f.dev, at::kFloat);
    c10::DeviceGuard guard(f.dev);
    Tensor out = empty({f.pop, f.gp_len}, at::kFloat, f.dev);
    check_rc(evogp_hip_point_mutate((int)f.pop, (int)f.gp_len, (int)mode, (float)rate, (float)intensity, per_node ? 1 : 0, modify_output ? 1 : 0,
                                    fix_roulette ? 1 : 0, (int)skip_rows, (int)input_len, (int)output_len, (int)const_samples.size(0), seed, call, f.value,
                                    f.type, f.size, roulette_ufuncs.data_ptr<float>(), roulette_bfuncs.data_ptr<float>(), roulette_tfuncs.data_ptr<float>(),
                                    const_samples.data_ptr<float>(), out.data_ptr<float>(), current_stream(f.dev)),
             "point_mutate");
    return out;
}

}  // namespace

// schemas of the reference, verbatim (torch_wrapper.cu:294-298)
TORCH_LIBRARY(evogp_cuda, m) {
    m.def("tree_generate(int i1, int i2, int i3, int i4, int i5, float f1, float f2, Tensor t1, Tensor t2, Tensor t3, Tensor t4) -> (Tensor t5, Tensor t6, Tensor t7)");
    m.def("tree_mutate(int i1, int i2, Tensor t1, Tensor t2, Tensor t3, Tensor t4, Tensor t5, Tensor t6, Tensor t7) -> (Tensor t8, Tensor t9, Tensor t10)");
    m.def("tree_crossover(int i1, int i2, int i3, Tensor t1, Tensor t2, Tensor t3, Tensor t4, Tensor t5, Tensor t6, Tensor t7) -> (Tensor t8, Tensor t9, Tensor t10)");
    m.def("tree_evaluate(int i1, int i2, int i3, int i4, Tensor t1, Tensor t2, Tensor t3, Tensor t4) -> Tensor t5");
    m.def("tree_SR_fitness(int i1, int i2, int i3, int i4, int i5, bool b1, Tensor t1, Tensor t2, Tensor t3, Tensor t4, Tensor t5, int i6) -> Tensor t6");
}

TORCH_LIBRARY_IMPL(evogp_cuda, CUDA, m) {
    m.impl("tree_generate", &tree_generate);
    m.impl("tree_mutate", &tree_mutate);
    m.impl("tree_crossover", &tree_crossover);
    m.impl("tree_evaluate", &tree_evaluate);
    m.impl("tree_SR_fitness", &tree_SR_fitness);
}

// the engine's record buffers come out of torch's caching allocator: torch.cuda.memory_allocated() / memory_summary() show them
// (include/evogp_hip.h evogp_hip_set_allocator; EVOGP_TORCH_ALLOCATOR=0: plain hipMalloc as in rounds 1-4)
static void *torch_pool_alloc(size_t bytes) {
    try {
        // Not while ANY stream of this thread's device is being captured: raw_alloc may then hand out memory of the
        // capture's private pool, and the device-wide wait the engine makes before it first touches a block would invalidate the
        // capture.  nullptr: the engine takes the call on kernels that need no record buffer.  (Blocks are returned to the pool only
        // by evogp_hip_release_workspaces, after a device-wide wait.)
        if (c10::hip::currentStreamCaptureStatusMayInitCtx() != c10::hip::CaptureStatus::None) return nullptr;
        return c10::hip::HIPCachingAllocator::raw_alloc(bytes);
    } catch (...) {
        return nullptr;
    }
}
static void torch_pool_free(void *ptr) { c10::hip::HIPCachingAllocator::raw_delete(ptr); }
static const int installed_allocator = [] {
    const char *e = getenv("EVOGP_TORCH_ALLOCATOR");
    return (e && e[0] == '0') ? 0 : evogp_hip_set_allocator(&torch_pool_alloc, &torch_pool_free);
}();

TORCH_LIBRARY(evogp_hip, m) {
    m.def("tree_generate_offset(int pop_size, int gp_len, int var_len, int out_len, int const_samples_len, float out_prob, float const_prob,"
          " Tensor keys, Tensor depth2leaf_probs, Tensor roulette_funcs, Tensor const_samples, int tree_index_offset)"
          " -> (Tensor value, Tensor node_type, Tensor subtree_size)");
    m.def("tree_generate_masked(int pop_size, int gp_len, int var_len, int out_len, int const_samples_len, float out_prob, float const_prob,"
          " Tensor keys, Tensor depth2leaf_probs, Tensor roulette_funcs, Tensor const_samples, int tree_index_offset,"
          " Tensor active_word, int active_below) -> (Tensor value, Tensor node_type, Tensor subtree_size)");
    m.def("tree_batch_evaluate(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables) -> Tensor results");
    m.def("tree_batch_argmax_count(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables, Tensor labels) -> Tensor counts");
    m.def("tree_batch_class_stats(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables, Tensor labels, Tensor? groups, int n_groups) -> (Tensor hits, Tensor predicted, Tensor loss)");
    m.def("tree_evaluate_prepare(int pop_size, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type, Tensor subtree_size)"
          " -> (Tensor workspace, Tensor info)");
    m.def("tree_evaluate_prepared(int pop_size, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type, Tensor subtree_size,"
          " Tensor workspace, bool with_fallback, Tensor variables) -> Tensor results");
    m.def("random_words(int seed, int generation, int rows, int n_cols, int lo, int hi, Device device) -> Tensor");
    m.def("fitness_scores(Tensor errors, bool negate) -> Tensor");
    m.def("select_survivors(Tensor fitness, int n_elite, int n_keep) -> Tensor");
    m.def("tournament_select(Tensor fitness, int n_tournaments, int t_size, int seed, int generation) -> Tensor");
    m.def("breed_default(int pop_size, int gp_len, int n_elite, int n_surv, Tensor value, Tensor node_type, Tensor subtree_size,"
          " Tensor order, Tensor rnd, int mutate_below, Tensor donor_value, Tensor donor_type, Tensor donor_size,"
          " bool want_decisions) -> (Tensor value, Tensor node_type, Tensor subtree_size, Tensor decisions)");
    m.def("breed_default_rows(int pop_size, int gp_len, int n_elite, int n_surv, Tensor value, Tensor node_type, Tensor subtree_size,"
          " Tensor order, Tensor rnd, int mutate_below, Tensor donor_value, Tensor donor_type, Tensor donor_size,"
          " int row_begin, int row_count) -> (Tensor value, Tensor node_type, Tensor subtree_size)");
    m.def("breed_rows(int pop_size, int gp_len, Tensor value, Tensor node_type, Tensor subtree_size, Tensor elite_rows, Tensor parent_rows,"
          " Tensor rnd, int mutate_below, Tensor donor_value, Tensor donor_type, Tensor donor_size, int row_begin, int row_count)"
          " -> (Tensor value, Tensor node_type, Tensor subtree_size)");
    m.def("breed_rows_hashed(int pop_size, int gp_len, Tensor value, Tensor node_type, Tensor subtree_size, Tensor elite_rows, Tensor parent_rows,"
          " int seed, int generation, int mutate_below, Tensor donor_value, Tensor donor_type, Tensor donor_size, int row_begin, int row_count)"
          " -> (Tensor value, Tensor node_type, Tensor subtree_size)");
    m.def("structural_mutate(int mode, float rate, int max_size, bool inner_is_offset, int skip_rows, int seed, int call, Tensor value, Tensor node_type,"
          " Tensor subtree_size, bool want_decisions) -> (Tensor value, Tensor node_type, Tensor subtree_size, Tensor decisions)");
    m.def("insert_mutate(int mutate_below, int skip_rows, int seed, int call, Tensor value, Tensor node_type, Tensor subtree_size, Tensor donor_value,"
          " Tensor donor_type, Tensor donor_size, bool want_decisions) -> (Tensor value, Tensor node_type, Tensor subtree_size, Tensor decisions)");
    m.def("point_mutate(int mode, float rate, float intensity, bool per_node, bool modify_output, bool fix_roulette, int skip_rows, int input_len, int output_len,"
          " int seed, int call, Tensor value, Tensor node_type, Tensor subtree_size, Tensor roulette_ufuncs, Tensor roulette_bfuncs, Tensor roulette_tfuncs,"
          " Tensor const_samples) -> Tensor");
    m.def("tree_generate_masked_hashed(int pop_size, int gp_len, int var_len, int out_len, int const_samples_len, float out_prob, float const_prob,"
          " Tensor depth2leaf_probs, Tensor roulette_funcs, Tensor const_samples, int tree_index_offset, int seed, int generation, int active_below)"
          " -> (Tensor value, Tensor node_type, Tensor subtree_size)");
    m.def("tree_SR_fitness_masked(int pop_size, int data_points, int gp_len, int var_len, int out_len, bool use_mse, Tensor value,"
          " Tensor node_type, Tensor subtree_size, Tensor variables, Tensor labels, int kernel_type, int func_mask) -> Tensor");
    m.def("tree_SR_gradient(int pop_size, int data_points, int gp_len, int var_len, int out_len, bool use_mse, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y) -> (Tensor loss, Tensor grad)");
    m.def("tree_SR_const_step(int phase, int out_len, Tensor(a!) value, Tensor node_type, Tensor subtree_size, Tensor(b!) value_cand,"
          " Tensor(c!) loss, Tensor(d!) grad, Tensor loss_cand, Tensor grad_cand, Tensor(e!) step) -> ()");
    m.def("tree_SR_case_errors(int pop_size, int data_points, int gp_len, int var_len, int out_len, bool use_mse, Tensor value,"
          " Tensor node_type, Tensor subtree_size, Tensor variables, Tensor labels) -> Tensor");
    m.def("lexicase_select(Tensor errors, Tensor eps, int n_events, int seed, int generation) -> Tensor");
    m.def("pareto_rank(Tensor err, Tensor cx, int cx_bound) -> (Tensor front, Tensor crowding, Tensor order)");
    m.def("nsga2_select(Tensor order, int pool, int n, int t_size, int seed, int generation) -> Tensor");
    m.def("tree_SR_subtree_errors(int pop_size, int data_points, int gp_len, int var_len, int out_len, bool use_mse, Tensor value,"
          " Tensor node_type, Tensor subtree_size, Tensor X, Tensor y) -> (Tensor node_err, Tensor node_const)");
    m.def("tree_prune(int out_len, bool hoist, bool fold, Tensor value, Tensor node_type, Tensor subtree_size, Tensor node_err,"
          " Tensor node_const) -> (Tensor value, Tensor node_type, Tensor subtree_size, Tensor root_pos, Tensor loss)");
    m.def("tree_SR_normal_eq(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y) -> (Tensor loss, Tensor normal)");
    m.def("tree_SR_lm_step(int phase, Tensor(a!) value, Tensor node_type, Tensor subtree_size, Tensor(b!) value_cand, Tensor(c!) loss,"
          " Tensor(d!) normal, Tensor loss_cand, Tensor normal_cand, Tensor(e!) damping) -> ()");
    m.def("tree_hash(Tensor value, Tensor node_type, Tensor subtree_size) -> Tensor");
    m.def("tree_classes(Tensor value, Tensor node_type, Tensor subtree_size, Tensor hash) -> Tensor");
    m.def("tree_SR_semantic_hash(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables) -> Tensor");
    m.def("tree_SR_semantic_classes(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables, Tensor hash) -> Tensor");
    m.def("tree_SR_subtree_signatures(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables) -> Tensor");
    m.def("tree_SR_subtree_introns(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor variables, Tensor sig) -> Tensor");
    m.def("tree_remove_introns(Tensor value, Tensor node_type, Tensor subtree_size, Tensor rep) -> (Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor removed)");
    m.def("tree_SR_pair_moments(Tensor value, Tensor node_type, Tensor subtree_size, Tensor mate_value, Tensor mate_type, Tensor mate_size,"
          " Tensor variables, Tensor? labels, Tensor first, Tensor candidates) -> (Tensor own, Tensor moments)");
    m.def("subtree_library_select(Tensor sig, Tensor size, int min_size, int max_size, int k) -> (Tensor member, Tensor count, Tensor n_classes)");
    m.def("tree_SR_linear_scaling(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y) -> (Tensor loss, Tensor coef)");
    m.def("tree_SR_weighted_loss(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y, Tensor? weights, int loss_kind, float loss_param) -> Tensor");
    m.def("tree_SR_weighted_scaling(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y, Tensor? weights) -> (Tensor loss, Tensor coef)");
    m.def("tree_SR_weighted_gradient(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y, Tensor? weights, int loss_kind, float loss_param) -> (Tensor loss, Tensor grad)");
    m.def("tree_SR_weighted_normal_eq(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y, Tensor? weights) -> (Tensor loss, Tensor normal)");
    m.def("tree_SR_gene_fitness(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y) -> (Tensor loss, Tensor coef)");
    m.def("tree_SR_gene_moments(int pop_size, int data_points, int gp_len, int var_len, int out_len, Tensor value, Tensor node_type,"
          " Tensor subtree_size, Tensor X, Tensor y) -> (Tensor loss, Tensor coef, Tensor moments)");
    m.def("tree_wrap_linear(int out_gp_len, Tensor value, Tensor node_type, Tensor subtree_size, Tensor coef)"
          " -> (Tensor value, Tensor node_type, Tensor subtree_size, Tensor applied)");
    m.def("tree_intervals(Tensor value, Tensor node_type, Tensor subtree_size, Tensor lower, Tensor upper) -> (Tensor lo, Tensor hi, Tensor flags)");
    m.def("tree_derivative_intervals(Tensor value, Tensor node_type, Tensor subtree_size, Tensor lower, Tensor upper, Tensor wrt) -> (Tensor vlo, Tensor vhi, Tensor vflags, Tensor dlo, Tensor dhi, Tensor dflags)");
    m.def("tree_SR_input_gradient(Tensor value, Tensor node_type, Tensor subtree_size, Tensor X, int[] wrt) -> (Tensor pred, Tensor dpred)");
    m.def("tree_SR_derivative_loss(Tensor value, Tensor node_type, Tensor subtree_size, Tensor X, Tensor y, Tensor? dlabels, int[] wrt,"
          " Tensor? dmin, Tensor? dmax) -> (Tensor loss, Tensor violations)");
    m.def("tree_SR_desired(Tensor value, Tensor node_type, Tensor subtree_size, Tensor X, Tensor y, Tensor pos) -> (Tensor desired, Tensor state, Tensor status)");
    m.def("tree_SR_backprop_match(Tensor value, Tensor node_type, Tensor subtree_size, Tensor X, Tensor y, Tensor pos, Tensor lib)"
          " -> (Tensor best, Tensor dist, Tensor const, Tensor const_dist, Tensor counts, Tensor status)");
    m.def("tree_SR_desired_mid(Tensor value, Tensor node_type, Tensor subtree_size, Tensor mate_value, Tensor mate_type, Tensor mate_size, Tensor X,"
          " Tensor pos, Tensor mate) -> (Tensor desired, Tensor state, Tensor status)");
    m.def("tree_SR_agx_match(Tensor value, Tensor node_type, Tensor subtree_size, Tensor mate_value, Tensor mate_type, Tensor mate_size, Tensor X,"
          " Tensor pos, Tensor mate, Tensor lib) -> (Tensor best, Tensor dist, Tensor const, Tensor const_dist, Tensor counts, Tensor status)");
    m.def("tree_dimensions(Tensor value, Tensor node_type, Tensor subtree_size, Tensor var_units, Tensor label_units, bool check_root) -> (Tensor units, Tensor flags, Tensor violations)");
    m.def("tree_structure(Tensor value, Tensor node_type, Tensor subtree_size, Tensor cost, Tensor operand_limit, Tensor rule_outer, Tensor rule_inner, Tensor rule_limit, int max_depth, int max_complexity)"
          " -> (Tensor complexity, Tensor height, Tensor depth, Tensor nest, Tensor flags, Tensor violations)");
}

TORCH_LIBRARY_IMPL(evogp_hip, CompositeExplicitAutograd, m) { m.impl("random_words", &random_words); }  // no tensor argument to dispatch on

TORCH_LIBRARY_IMPL(evogp_hip, CUDA, m) {
    m.impl("tree_generate_offset", &tree_generate_offset);
    m.impl("tree_generate_masked", &tree_generate_masked);
    m.impl("tree_batch_evaluate", &tree_batch_evaluate);
    m.impl("tree_batch_argmax_count", &tree_batch_argmax_count);
    m.impl("tree_batch_class_stats", &tree_batch_class_stats);
    m.impl("tree_evaluate_prepare", &tree_evaluate_prepare);
    m.impl("tree_evaluate_prepared", &tree_evaluate_prepared);
    m.impl("breed_default", &breed_default);
    m.impl("breed_default_rows", &breed_default_rows);
    m.impl("breed_rows", &breed_rows);
    m.impl("breed_rows_hashed", &breed_rows_hashed);
    m.impl("tree_generate_masked_hashed", &tree_generate_masked_hashed);
    m.impl("structural_mutate", &structural_mutate);
    m.impl("insert_mutate", &insert_mutate);
    m.impl("point_mutate", &point_mutate);
    m.impl("tree_SR_fitness_masked", &tree_SR_fitness_masked);
    m.impl("select_survivors", &select_survivors);
    m.impl("fitness_scores", &fitness_scores);
    m.impl("tournament_select", &tournament_select);
    m.impl("tree_SR_gradient", &tree_SR_gradient);
    m.impl("tree_SR_const_step", &tree_SR_const_step);
    m.impl("tree_SR_case_errors", &tree_SR_case_errors);
    m.impl("lexicase_select", &lexicase_select);
    m.impl("pareto_rank", &pareto_rank);
    m.impl("nsga2_select", &nsga2_select);
    m.impl("tree_SR_subtree_errors", &tree_SR_subtree_errors);
    m.impl("tree_prune", &tree_prune);
    m.impl("tree_SR_normal_eq", &tree_SR_normal_eq);
    m.impl("tree_SR_lm_step", &tree_SR_lm_step);
    m.impl("tree_hash", &tree_hash);
    m.impl("tree_classes", &tree_classes);
    m.impl("tree_SR_semantic_hash", &tree_SR_semantic_hash);
    m.impl("tree_SR_semantic_classes", &tree_SR_semantic_classes);
    m.impl("tree_SR_subtree_signatures", &tree_SR_subtree_signatures);
    m.impl("subtree_library_select", &subtree_library_select);
    m.impl("tree_SR_subtree_introns", &tree_SR_subtree_introns);
    m.impl("tree_remove_introns", &tree_remove_introns);
    m.impl("tree_SR_pair_moments", &tree_SR_pair_moments);
    m.impl("tree_SR_linear_scaling", &tree_SR_linear_scaling);
    m.impl("tree_SR_weighted_loss", &tree_SR_weighted_loss);
    m.impl("tree_SR_weighted_scaling", &tree_SR_weighted_scaling);
    m.impl("tree_SR_weighted_gradient", &tree_SR_weighted_gradient);
    m.impl("tree_SR_weighted_normal_eq", &tree_SR_weighted_normal_eq);
    m.impl("tree_SR_gene_fitness", &tree_SR_gene_fitness);
    m.impl("tree_SR_gene_moments", &tree_SR_gene_moments);
    m.impl("tree_wrap_linear", &tree_wrap_linear);
    m.impl("tree_intervals", &tree_intervals);
    m.impl("tree_derivative_intervals", &tree_derivative_intervals);
    m.impl("tree_SR_input_gradient", &tree_SR_input_gradient);
    m.impl("tree_SR_derivative_loss", &tree_SR_derivative_loss);
    m.impl("tree_SR_desired", &tree_SR_desired);
    m.impl("tree_SR_backprop_match", &tree_SR_backprop_match);
    m.impl("tree_SR_desired_mid", &tree_SR_desired_mid);
    m.impl("tree_SR_agx_match", &tree_SR_agx_match);
    m.impl("tree_dimensions", &tree_dimensions);
    m.impl("tree_structure", &tree_structure);
}
