// Driver part: CRC-32 and Adler-32 of ranges of the resident input (zmx_checksum.h).  Holds zmx_checksum
// and zmx_checksums.  Needs drv_context.h (zmx_ctx, PoolScope).
#pragma once

extern "C" {
static bool IsChecksumKind(int kind) { return kind == ZMX_CRC32 || kind == ZMX_ADLER32; }
static_assert(sizeof(zamd::ChecksumPiece) == 12, "three words per piece");
// a range of `len` bytes from its pieces
static uint32_t FinishChecksum(int kind, const zamd::ChecksumPiece* pieces, size_t npieces, uint64_t len) {
  return kind == ZMX_CRC32 ? zamd::FinishCrc32(pieces, npieces, len) : zamd::FinishAdler32(pieces, npieces, len);
}

int zmx_checksum(zmx_ctx* c, int kind, size_t begin, size_t end, uint32_t* value) {
  if (!IsChecksumKind(kind)) return FailMsg("zmx_checksum: unknown kind");
  if (begin > end || end > c->insize) return FailMsg("zmx_checksum: range outside the resident input");
  const size_t n = end - begin;
  const size_t npieces = (n + zamd::kChecksumPieceBytes - 1) / zamd::kChecksumPieceBytes;
  std::vector<zamd::ChecksumPiece> pieces(npieces);
  if (npieces) {
    DEVICE_ENTRY(c->device);
    PoolScope tmp(c);
    u32* d_out = nullptr;
    HIPCHK(tmp.AllocT(&d_out, 3 * npieces, "d_out"));
    ChecksumParams P;
    P.in = c->d_in;
    P.begin = static_cast<long long>(begin);
    P.end = static_cast<long long>(end);
    P.out = d_out;
    zamd::ChecksumTreePowers(P.xpow);
    hipLaunchKernelGGL(k_checksum, dim3(static_cast<unsigned>(npieces)), dim3(256), 0, c->stream, P);
    KCHK(c, "k_checksum");
    HIPCHK(hipMemcpyAsync(pieces.data(), d_out, npieces * sizeof(zamd::ChecksumPiece), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  *value = FinishChecksum(kind, pieces.data(), npieces, n);
  return 0;
}

// zmx_checksum of n ranges in one launch: the 256 KiB pieces of every range, each range's listed from its end, go through
// k_checksums together and are put together per range on the host.
int zmx_checksums(zmx_ctx* c, int kind, size_t n, const uint64_t* begin, const uint64_t* end, uint32_t* values) {
  if (!IsChecksumKind(kind)) return FailMsg("zmx_checksums: unknown kind");
  if (n == 0) return 0;
  if (!begin || !end || !values) return FailMsg("zmx_checksums: null array");
  std::vector<size_t> first(n + 1, 0);
  for (size_t r = 0; r < n; ++r) {
    if (begin[r] > end[r] || end[r] > c->insize) return FailMsg("zmx_checksums: range outside the resident input");
    first[r + 1] = first[r] + (end[r] - begin[r] + zamd::kChecksumPieceBytes - 1) / zamd::kChecksumPieceBytes;
  }
  const size_t npieces = first[n];
  if (npieces > 0x7fffffffull) return FailMsg("zmx_checksums: too many pieces for one launch");
  std::vector<zamd::ChecksumPiece> pieces(npieces);
  if (npieces) {
    std::vector<long long> tab(2 * npieces);
    for (size_t r = 0; r < n; ++r) {
      for (size_t j = first[r]; j < first[r + 1]; ++j) {
        tab[2 * j] = static_cast<long long>(begin[r]);
        tab[2 * j + 1] = static_cast<long long>(end[r]) - static_cast<long long>((j - first[r]) * zamd::kChecksumPieceBytes);
      }
    }
    DEVICE_ENTRY(c->device);
    PoolScope tmp(c);
    u32* d_out = nullptr;
    long long* d_tab = nullptr;
    HIPCHK(tmp.AllocT(&d_out, 3 * npieces, "d_out"));
    HIPCHK(tmp.Upload(&d_tab, tab.data(), tab.size(), "d_tab"));
    ChecksumsParams P;
    P.in = c->d_in;
    P.pieces = d_tab;
    P.out = d_out;
    zamd::ChecksumTreePowers(P.xpow);
    hipLaunchKernelGGL(k_checksums, dim3(static_cast<unsigned>(npieces)), dim3(256), 0, c->stream, P);
    KCHK(c, "k_checksums");
    HIPCHK(hipMemcpyAsync(pieces.data(), d_out, npieces * sizeof(zamd::ChecksumPiece), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  for (size_t r = 0; r < n; ++r) {
    values[r] = FinishChecksum(kind, pieces.data() + first[r], first[r + 1] - first[r], end[r] - begin[r]);
  }
  return 0;
}
}  // extern "C"
