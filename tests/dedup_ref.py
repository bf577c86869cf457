"""numpy restatement of structural duplicate detection (include/evogp_hip.h evogp_hip_tree_hash / evogp_hip_tree_classes,
csrc/dedup.hip): the hash, the equality of two rows and ``class_id``.

    n = size[t][0]; a row with n < 1 or n > gp_len is OUT OF RANGE: a class of its own, hash 0
    in-range rows are EQUAL when their n are equal and value bits, type words and size words agree on every i < n
    hash = mix64((sum_{i<n} mix64(w_i ^ ((i + 1) * GOLD))) + n) mod 2^64,  w_i = (uint64)(uint16)type[i] << 32 | bits(value[i])
    class_id[t] = the smallest tree index whose row equals row t
"""
import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)


def mix64(x):
    """the splitmix64 finaliser (csrc/evogp_defs.hpp mix64) on a uint64 array"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def in_range(size_row, gp_len):
    return 1 <= int(size_row[0]) <= gp_len


def row_hash(value_row, type_row, size_row):
    L = value_row.shape[0]
    if not in_range(size_row, L):
        return np.uint64(0)
    n = int(size_row[0])
    bits = np.ascontiguousarray(value_row[:n], np.float32).view(np.uint32).astype(np.uint64)
    w = (np.ascontiguousarray(type_row[:n], np.int16).view(np.uint16).astype(np.uint64) << np.uint64(32)) | bits
    with np.errstate(over="ignore"):
        keyed = mix64(w ^ (np.arange(1, n + 1, dtype=np.uint64) * GOLD))
        return mix64(np.array([keyed.sum(dtype=np.uint64) + np.uint64(n)], np.uint64))[0]


def tree_hash(value, type_, size):
    """uint64 (pop,)"""
    return np.array([row_hash(value[t], type_[t], size[t]) for t in range(value.shape[0])], np.uint64)


def rows_equal(value, type_, size, a, b):
    """the equality of rows a and b (a row equals itself; an out-of-range row equals no other)"""
    if a == b:
        return True
    L = value.shape[1]
    if not (in_range(size[a], L) and in_range(size[b], L)):
        return False
    n = int(size[a, 0])
    if int(size[b, 0]) != n:
        return False
    return (np.array_equal(value[a, :n].view(np.uint32), value[b, :n].view(np.uint32)) and np.array_equal(type_[a, :n], type_[b, :n])
            and np.array_equal(size[a, :n], size[b, :n]))


def class_id(value, type_, size):
    """int32 (pop,): the smallest index of an equal row, found through a dictionary of the live prefixes' bytes"""
    value, type_, size = (np.ascontiguousarray(a) for a in (value, type_, size))
    pop, L = value.shape
    seen = {}
    out = np.empty(pop, np.int32)
    for t in range(pop):
        if not in_range(size[t], L):
            out[t] = t
            continue
        n = int(size[t, 0])
        key = (n, value[t, :n].tobytes(), type_[t, :n].tobytes(), size[t, :n].tobytes())
        out[t] = seen.setdefault(key, t)
    return out
