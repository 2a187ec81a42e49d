// Structural check of a host CSR hand-off (mg_csr_check, include/mg_hip.h).  Pure host code, no HIP call: it needs
// nothing but the arrays, and runs before anything of a hand-off reaches the device -- the set-up kernels (csr_scan,
// csr_to_ell, jacobi_split) index the caller's arrays unchecked.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace mgk {

// "" if (indptr, indices) describe an n_rows x n_cols CSR pattern of nnz entries, else what is wrong with it, rows and
// columns in the caller's own numbering.  Two passes, each linear: the row pointers first -- only once they are known to
// start at 0, never decrease and end at nnz may a row's entries be read at all -- then the column indices, on up to
// eight threads.
inline std::string csr_check(int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, int indptr_is_64,
                             const int32_t* indices, bool allow_duplicates) {
    if (n_rows < 0 || n_cols < 0 || nnz < 0) return "bad matrix dimensions";
    if (!indptr || (nnz > 0 && !indices)) return "null CSR arrays";
    const int64_t* const p64 = static_cast<const int64_t*>(indptr);
    const int32_t* const p32 = static_cast<const int32_t*>(indptr);
    auto at = [&](int64_t i) -> int64_t { return indptr_is_64 ? p64[i] : (int64_t)p32[i]; };
    if (at(0) != 0) return "CSR indptr[0] is " + std::to_string(at(0)) + ", not 0";
    int64_t prev = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t next = at(r + 1);
        if (next < prev)
            return "CSR indptr decreases at row " + std::to_string(r) + " (indptr[" + std::to_string(r) + "] = " +
                   std::to_string(prev) + ", indptr[" + std::to_string(r + 1) + "] = " + std::to_string(next) + ")";
        prev = next;
    }
    if (prev != nnz)
        return "CSR indptr[n_rows] is " + std::to_string(prev) + ", but nnz is " + std::to_string(nnz);
    // the entries: columns in range and, unless allowed, no column twice in a row.  Duplicates in one pass, without
    // sorting a row: stamp[c] = 1 + the last row that touched column c.  Large matrices are cut into contiguous row ranges
    // of about equal entries, one thread each with a stamp array of its own (zero pages until touched: a thread touches the
    // columns near its rows); the lowest range that found something reports, so the message is the one a single pass gives.
    auto scan = [&](int64_t r0, int64_t r1, std::string& why) {
        // (calloc, not a vector: the pages stay untouched zero pages until a column is stamped)
        std::unique_ptr<int64_t, decltype(&std::free)> owner(
            allow_duplicates ? nullptr : static_cast<int64_t*>(std::calloc((size_t)std::max<int64_t>(1, n_cols), sizeof(int64_t))), &std::free);
        int64_t* const stamp = owner.get();
        if (!allow_duplicates && !stamp) {
            why = "out of host memory in the CSR check";
            return;
        }
        int64_t q = at(r0);
        for (int64_t r = r0; r < r1; ++r) {
            for (const int64_t e = at(r + 1); q < e; ++q) {
                const int64_t col = indices[q];
                if (col < 0 || col >= n_cols) {
                    why = "CSR row " + std::to_string(r) + " holds column index " + std::to_string(col) + " outside [0, " +
                          std::to_string(n_cols) + ")";
                    return;
                }
                if (allow_duplicates) continue;
                if (stamp[(size_t)col] == r + 1) {
                    why = "CSR row " + std::to_string(r) + " holds column " + std::to_string(col) +
                          " twice; sum duplicates before the hand-off (A.sum_duplicates())";
                    return;
                }
                stamp[(size_t)col] = r + 1;
            }
        }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = nnz < (int64_t(1) << 20) ? 1 : (int)std::min<int64_t>({8, hw ? (int64_t)hw : 1, n_rows});
    if (nthreads <= 1) {
        std::string why;
        scan(0, n_rows, why);
        return why;
    }
    std::vector<int64_t> cut((size_t)nthreads + 1, n_rows);
    cut[0] = 0;
    for (int t = 1; t < nthreads; ++t) {            // first row whose entries start at or after t / nthreads of nnz
        const int64_t want = nnz / nthreads * t;
        int64_t lo = cut[(size_t)t - 1], hi = n_rows;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (at(mid) < want) lo = mid + 1; else hi = mid;
        }
        cut[(size_t)t] = lo;
    }
    std::vector<std::string> why((size_t)nthreads);
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t)
        pool.emplace_back([&, t]() { scan(cut[(size_t)t], cut[(size_t)t + 1], why[(size_t)t]); });
    scan(cut[0], cut[1], why[0]);
    for (auto& th : pool) th.join();
    for (const auto& w : why)
        if (!w.empty()) return w;
    return "";
}

}  // namespace mgk
