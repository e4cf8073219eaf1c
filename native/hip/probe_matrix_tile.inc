using TileKernel = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*);

// matrix_tile_kernel<P, opsel / 4, opsel % 4> for every opsel of the sequence: the byte selects
// are immediates of the instruction. The unscaled paths have the one instantiation <P, 0, 0>.
template <int P, int... I>
TileKernel opsel_kernel(std::integer_sequence<int, I...>, int opsel) {
  static constexpr TileKernel table[] = {matrix_tile_kernel<P, I / 4, I % 4>...};
  return table[sizeof...(I) == 1 ? 0 : opsel];
}

template <int P>
TileKernel path_kernel(int opsel) {
  return opsel_kernel<P>(std::make_integer_sequence<int, sp::path_scaled(P) ? 16 : 1>{}, opsel);
}

template <int... P>
TileKernel tile_kernel(std::integer_sequence<int, P...>, int p, int opsel) {
  static constexpr TileKernel (*table[])(int) = {path_kernel<P>...};
  return table[p](opsel);
}

// One instruction of path `p` on the caller's codes: a_codes is A[row][k] (dim x K, row-major),
// b_codes is B[k][col] (K x dim), scale_a is [row][k block] and scale_b [k block][col] (E8M0,
// scaled paths only), opsel_a / opsel_b the scale register's byte that carries them (the
// other bytes get another scale). Returns the tile's words, row-major (path_expected_words).
std::vector<uint32_t> matrix_tile(int p, const std::vector<uint64_t>& a_codes, const std::vector<uint64_t>& b_codes,
                                  const std::vector<uint32_t>& scale_a, const std::vector<uint32_t>& scale_b,
                                  int opsel_a, int opsel_b) {
  if (p < 0 || p >= sp::kNumPaths) throw std::invalid_argument("matrix_tile: unknown path");
  const int dim = sp::path_dim(p), K = sp::path_k(p), cb = sp::path_code_bits(p), rowdw = sp::path_row_dwords(p);
  const size_t n = static_cast<size_t>(dim) * K;
  if (a_codes.size() != n || b_codes.size() != n)
    throw std::invalid_argument("matrix_tile: A is dim x K codes and B is K x dim codes");
  const size_t n_scale = sp::path_scaled(p) ? static_cast<size_t>(dim) * 2 : 0;
  if (scale_a.size() != n_scale || scale_b.size() != n_scale)
    throw std::invalid_argument("matrix_tile: scales are dim x 2 and 2 x dim on the scaled paths, absent elsewhere");
  if (opsel_a < 0 || opsel_a > 3 || opsel_b < 0 || opsel_b > 3) throw std::invalid_argument("matrix_tile: opsel in 0..3");
  std::vector<uint32_t> A(static_cast<size_t>(dim) * rowdw, 0u), B(A.size(), 0u), SA(dim * 2, 0u), SB(dim * 2, 0u);
  auto put = [&](std::vector<uint32_t>& v, int idx, int k, uint64_t code) {
    if (cb < 64 && (code >> cb)) throw std::invalid_argument("matrix_tile: a code wider than the format");
    size_t bit = static_cast<size_t>(idx) * rowdw * 32 + static_cast<size_t>(k) * cb;
    for (int i = 0; i < cb;) {
      const int sh = static_cast<int>(bit % 32), take = std::min(cb - i, 32 - sh);
      v[bit / 32] |= static_cast<uint32_t>((code >> i) & ((1ull << take) - 1)) << sh;
      i += take;
      bit += take;
    }
  };
  for (int i = 0; i < dim; ++i)
    for (int k = 0; k < K; ++k) {
      put(A, i, k, a_codes[static_cast<size_t>(i) * K + k]);
      put(B, i, k, b_codes[static_cast<size_t>(k) * dim + i]);
    }
  auto scale_dword = [](uint32_t scale, int byte) {
    if (scale > 0xfe) throw std::invalid_argument("matrix_tile: an E8M0 scale is 0..254");
    return ((scale ^ 1u) * 0x01010101u & ~(0xffu << (8 * byte))) | (scale << (8 * byte));
  };
  for (size_t i = 0; i < n_scale / 2; ++i)
    for (int blk = 0; blk < 2; ++blk) {
      SA[i * 2 + blk] = scale_dword(scale_a[i * 2 + blk], opsel_a);
      SB[i * 2 + blk] = scale_dword(scale_b[static_cast<size_t>(blk) * dim + i], opsel_b);
    }
  DevBuf<uint32_t> da(A.size()), db(B.size()), dsa(SA.size()), dsb(SB.size()), dc(sp::kTileWords);
  HIP_OK(hipMemcpy(da.p, A.data(), A.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db.p, B.data(), B.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dsa.p, SA.data(), SA.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dsb.p, SB.data(), SB.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dc.p, 0, sp::kTileWords * 4));
  hipLaunchKernelGGL(tile_kernel(AllPaths{}, p, opsel_a * 4 + opsel_b), dim3(1), dim3(64), 0, 0, da.p, db.p, dsa.p, dsb.p,
                     dc.p);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> c(sp::path_tile_words(p));
  HIP_OK(hipMemcpy(c.data(), dc.p, c.size() * 4, hipMemcpyDeviceToHost));
  return c;
}
