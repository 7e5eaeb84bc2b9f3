// trace_pack_host.hpp -- host-only encoder and decoder of the packed pad-trace rows, format "for64-bitplane-v1"
// (include/attpc_engine.h, "packed pad traces": attpc_trace_pack_host, attpc_trace_unpack).  Plain C++17, no HIP:
// compiled into libattpc_hip.so with abi.hip and, by tests/test_trace_pack_sanitizers.py, on its own under
// -fsanitize=address,undefined and -fsanitize=thread.
#pragma once
#include <stdint.h>

namespace attpc {

constexpr int TP_SAMPLES = 512;      // samples of a row (ATTPC_NUM_TB)
constexpr int TP_BLOCK = 64;         // samples of a block: one plane word
constexpr int TP_BLOCKS = TP_SAMPLES / TP_BLOCK;
constexpr int TP_MAX_WIDTH = 12;     // bit planes of a block at most
constexpr int TP_MAX_SAMPLE = 4095;
constexpr int TP_HEADER_BYTES = 2 * TP_BLOCKS;
constexpr int TP_MAX_ROW_BYTES = TP_HEADER_BYTES + 8 * TP_BLOCKS * TP_MAX_WIDTH;  // 784

// Results: 0 = done, 1 = refused (ATTPC_OK / ATTPC_E_INVALID), 4 = the bytes do not fit (ATTPC_E_CAPACITY).

// samples [n_rows][512], every one in 0 .. 4095 (else refused, nothing promised about the outputs) -> row_start
// [n_rows + 1] (written whenever it is given) and, while they fit byte_capacity, the records in bytes; *n_bytes = the
// bytes all rows take, also when they do not fit (result 4: bytes then holds the rows that fit in front).
int32_t trace_pack_host(int64_t n_rows, const int16_t* samples, int64_t* row_start, uint8_t* bytes, int64_t byte_capacity,
                        int64_t* n_bytes);

// The records row_start[r] .. row_start[r + 1] of bytes [n_bytes], r < n_rows -> samples [n_rows][512].  Every record
// is checked against its span before a byte of it beyond the header is read; refused: a span that is no multiple of
// 8, decreases, starts below 0 or ends past n_bytes, a width above 12, base + 2^w - 1 above 4095, a span other than
// 16 + 8 sum(w).  Nothing outside bytes [0, n_bytes), row_start [0, n_rows] and samples [0, n_rows * 512) is touched.
// n_threads as in unpack_host.hpp (one thread per 4 096 rows at most).
int32_t trace_unpack_host(const uint8_t* bytes, int64_t n_bytes, const int64_t* row_start, int64_t n_rows, int16_t* samples,
                          int n_threads);

}  // namespace attpc
