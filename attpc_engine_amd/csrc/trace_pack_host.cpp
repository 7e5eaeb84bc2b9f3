// trace_pack_host.cpp -- see trace_pack_host.hpp.  The words of a record are little-endian whatever the host is: they
// are put together from and taken apart into single bytes.  Decoder threads write disjoint row ranges of the caller's
// samples.
#include "trace_pack_host.hpp"

#include "host_threads.hpp"

#include <atomic>
#include <thread>
#include <vector>

namespace attpc {
namespace {

constexpr int32_t TP_OK = 0, TP_INVALID = 1, TP_CAPACITY = 4;

inline void put_u16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v & 0xffu);
  p[1] = (uint8_t)(v >> 8);
}
inline void put_u64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline uint32_t get_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint64_t get_u64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

inline int bit_length(uint32_t v) {
  int n = 0;
  for (; v; v >>= 1) ++n;
  return n;
}

// base | w << 12 of every block of a row, and the bytes of its record; false: a sample outside 0 .. 4095
bool row_headers(const int16_t* row, uint32_t* headers, int64_t* size) {
  int planes = 0;
  for (int b = 0; b < TP_BLOCKS; ++b) {
    int lo = TP_MAX_SAMPLE + 1, hi = -1;
    for (int i = 0; i < TP_BLOCK; ++i) {
      const int v = row[TP_BLOCK * b + i];
      if (v < 0 || v > TP_MAX_SAMPLE) return false;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    const int w = bit_length((uint32_t)(hi - lo));
    lo = std::min(lo, TP_MAX_SAMPLE + 1 - (1 << w));  // the base: the minimum, lowered where minimum + 2^w - 1 would pass 4095
    headers[b] = (uint32_t)lo | ((uint32_t)w << 12);
    planes += w;
  }
  *size = TP_HEADER_BYTES + 8 * (int64_t)planes;
  return true;
}

void write_record(const int16_t* row, const uint32_t* headers, uint8_t* rec) {
  for (int b = 0; b < TP_BLOCKS; ++b) put_u16(rec + 2 * b, headers[b]);
  uint8_t* word = rec + TP_HEADER_BYTES;
  for (int b = 0; b < TP_BLOCKS; ++b) {
    const int base = (int)(headers[b] & 0xfffu), w = (int)(headers[b] >> 12);
    for (int k = 0; k < w; ++k, word += 8) {
      uint64_t plane = 0;
      for (int i = 0; i < TP_BLOCK; ++i) plane |= (uint64_t)(((uint32_t)(row[TP_BLOCK * b + i] - base) >> k) & 1u) << i;
      put_u64(word, plane);
    }
  }
}

// records lo .. hi - 1; false: one of them is refused
bool unpack_slice(const uint8_t* bytes, int64_t n_bytes, const int64_t* row_start, int64_t lo, int64_t hi, int16_t* samples) {
  for (int64_t r = lo; r < hi; ++r) {
    const int64_t at = row_start[r], end = row_start[r + 1];
    if (at < 0 || end < at || end > n_bytes || (at & 7) || (end & 7) || end - at < TP_HEADER_BYTES) return false;
    const uint8_t* rec = bytes + at;
    int base[TP_BLOCKS], width[TP_BLOCKS];
    int planes = 0;
    for (int b = 0; b < TP_BLOCKS; ++b) {
      const uint32_t h = get_u16(rec + 2 * b);
      base[b] = (int)(h & 0xfffu);
      width[b] = (int)(h >> 12);
      if (width[b] > TP_MAX_WIDTH || base[b] + (1 << width[b]) - 1 > TP_MAX_SAMPLE) return false;
      planes += width[b];
    }
    if (end - at != TP_HEADER_BYTES + 8 * (int64_t)planes) return false;
    const uint8_t* word = rec + TP_HEADER_BYTES;
    int16_t* out = samples + r * TP_SAMPLES;
    for (int b = 0; b < TP_BLOCKS; ++b) {
      uint16_t v[TP_BLOCK] = {0};
      for (int k = 0; k < width[b]; ++k, word += 8) {
        const uint64_t plane = get_u64(word);
        for (int i = 0; i < TP_BLOCK; ++i) v[i] = (uint16_t)(v[i] | (((plane >> i) & 1u) << k));
      }
      for (int i = 0; i < TP_BLOCK; ++i) out[TP_BLOCK * b + i] = (int16_t)(base[b] + v[i]);  // (<= base + 2^w - 1 <= 4095)
    }
  }
  return true;
}

}  // namespace

int32_t trace_pack_host(int64_t n_rows, const int16_t* samples, int64_t* row_start, uint8_t* bytes, int64_t byte_capacity,
                        int64_t* n_bytes) {
  if (n_rows < 0 || byte_capacity < 0 || (n_rows > 0 && !samples)) return TP_INVALID;
  int64_t at = 0;
  if (row_start) row_start[0] = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    uint32_t headers[TP_BLOCKS];
    int64_t size = 0;
    if (!row_headers(samples + r * TP_SAMPLES, headers, &size)) return TP_INVALID;
    if (bytes && at + size <= byte_capacity) write_record(samples + r * TP_SAMPLES, headers, bytes + at);
    at += size;
    if (row_start) row_start[r + 1] = at;
  }
  if (n_bytes) *n_bytes = at;
  return bytes && at > byte_capacity ? TP_CAPACITY : TP_OK;
}

int32_t trace_unpack_host(const uint8_t* bytes, int64_t n_bytes, const int64_t* row_start, int64_t n_rows, int16_t* samples,
                          int n_threads) {
  if (n_rows < 0 || n_bytes < 0) return TP_INVALID;
  if (n_rows == 0) return TP_OK;
  if (!row_start || !samples || (n_bytes > 0 && !bytes)) return TP_INVALID;
  n_threads = pick_threads(n_threads, n_rows, 4096);
  if (n_threads <= 1) return unpack_slice(bytes, n_bytes, row_start, 0, n_rows, samples) ? TP_OK : TP_INVALID;
  std::atomic<int> bad{0};
  std::vector<std::thread> pool;
  const int64_t per = (n_rows + n_threads - 1) / n_threads;
  auto work = [&](int t) {
    const int64_t lo = std::min<int64_t>(n_rows, per * t), hi = std::min<int64_t>(n_rows, lo + per);
    if (!unpack_slice(bytes, n_bytes, row_start, lo, hi, samples)) bad.store(1, std::memory_order_relaxed);
  };
  for (int t = 1; t < n_threads; ++t) pool.emplace_back(work, t);
  work(0);
  for (std::thread& th : pool) th.join();
  return bad.load() ? TP_INVALID : TP_OK;
}

}  // namespace attpc
