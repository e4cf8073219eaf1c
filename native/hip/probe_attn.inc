// The attention tenant of the interference calibration: O[b] (fp32) = softmax(Q[b] K[b]^T / sqrt(128)) V[b] for every
// head b, non-causal, head dimension 128, Q, K and V bf16 and row-major, by the online-softmax recurrence: S and P
// never touch memory. Two instantiations of one kernel: "wide" for prefill (sq a multiple of 128), bound by the
// matrix unit and the vector ALU between its two MFMA chains, and "split" for decode (sq a multiple of 32 below 128),
// which streams K and V once for a few queries and is memory-bound at any size. nanogpu/attn_host.h holds the tile
// sizes, the shape rules, the workgroup-to-(head, query tile) map and every index formed here;
// native/tests/attn_host_main.cpp checks them on the CPU.

namespace at = nanogpu::attn;

// ---------------------------------------------------------------------------- kernels

// x of lane ^ 32: what a query's two lanes exchange, by ds_bpermute_b32. __builtin_amdgcn_permlane32_swap with one
// value as both of its operands is not used: the compiler folded its two results into one (v_add_f32 v0, v165, v165
// after the swap), which lost the other half.
__device__ inline float other_half(float x) { return __shfl_xor(x, 32, 64); }

// The problem is worked transposed, so that a query is a lane column and its softmax state three scalars of a lane.
// Scores: S^T = K_blk . Q^T, a block of 32 kv rows by 8 MFMAs into one f32x16; Q^T's operands are eight consecutive d
// of one query row, loaded once from memory and kept in 8 registers of bf16x8; K's come from LDS with ds_read_b128.
// Lane l then holds 16 scores of query l & 31, and lane l ^ 32 the other 16: the block's maximum is 16 v_max and one
// exchange. The running max m stays in score units; p = exp2((s - m) c) with c = log2(e) / sqrt(128), so that the
// largest score gives exactly 1. The running sum stays per lane, and the two lanes of a query add theirs once, at
// the end. O^T += V_blk^T . P^T needs no movement of P: registers 8u .. 8u+7 of the scores, cast to bf16, are the B
// operand of k-step u as they stand, under a permutation of the kv index that V^T's A operand repeats
// (at::v_read_index), read from V row-major in LDS with two transposed reads. O^T of 32 queries x 128 d is four
// f32x16, rescaled by the lane's alpha = exp2((m_old - m_new) c) once a tile.
//
// Wide: wave w owns queries 32w .. 32w+31 and all four share each tile of 64 kv rows, two blocks whose scores are
// taken together, through two LDS stages with one barrier a tile as in gemm_bf16_kernel. Split: the four waves
// share 32 queries and split each tile of 128 rows, one block and one (m, l, O^T) each, through one LDS stage and two
// barriers a tile; after the last tile the four states are merged through the same LDS, each wave one quarter of d.
// No tail code: the host admits only shapes the tiles divide (at::shape_ok). No loop but the one over skv.
template <bool kSplit>
__global__ __launch_bounds__(at::kThreads, 2) void attn_bf16_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K,
                                                                    const uint16_t* __restrict__ V, float* __restrict__ O,
                                                                    int sq, int skv) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[at::kLdsElems];
  constexpr int kPasses = at::load_passes(kSplit), kBlocks = at::blocks_per_wave(kSplit), kStages = at::stages(kSplit);
  constexpr float kScale = static_cast<float>(1.4426950408889634 / 11.313708498984761);   // log2(e) / sqrt(128)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const at::PairAt at_ = at::pair_at(gm::tile_of_block(blockIdx.x, gridDim.x), sq);
  const int head = at_.head, qt = at_.qt;
  const int kv_tiles = skv / at::kv_tile(kSplit);

  bf16x8 q[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) q[s] = *reinterpret_cast<const bf16x8*>(Q + at::q_global_index(kSplit, head, qt, sq, wave, lane, s));

  u16x8 rk[kPasses], rv[kPasses];
  auto load_global = [&](int kt) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
      const size_t g = at::kv_global_index(kSplit, head, kt, skv, tid, i);
      rk[i] = *reinterpret_cast<const u16x8*>(K + g);
      rv[i] = *reinterpret_cast<const u16x8*>(V + g);
    }
  };
  auto store_lds = [&](int stage) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
      *reinterpret_cast<u16x8*>(&lds[at::k_lds_index(kSplit, stage, at::kv_load_row(tid, i), at::kv_load_chunk(tid))]) = rk[i];
      *reinterpret_cast<u16x8*>(&lds[at::v_lds_index(kSplit, stage, at::kv_load_row(tid, i), at::kChunk * at::kv_load_chunk(tid))]) = rv[i];
    }
  };
  auto read_tr = [&](int index) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4*)reinterpret_cast<bf16x4*>(&lds[index]));
  };

  f32x16 o[4] = {};
  float m = -1e30f, l = 0.f;   // a finite start: the first alpha is exp2 of a large negative number, 0, and no NaN
  load_global(0);
  store_lds(0);
  __syncthreads();
  for (int kt = 0; kt < kv_tiles; ++kt) {
    const int stage = kStages == 2 ? kt & 1 : 0;
    const bool more = kt + 1 < kv_tiles;
    if (more) load_global(kt + 1);

    f32x16 sc[kBlocks] = {};
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int b = 0; b < kBlocks; ++b) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&lds[at::k_read_index(kSplit, stage, wave, lane, b, s)]);
        sc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, q[s], sc[b], 0, 0, 0);
      }
    float mx = m;
#pragma unroll
    for (int b = 0; b < kBlocks; ++b)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) mx = fmaxf(mx, sc[b][reg]);
    mx = fmaxf(mx, other_half(mx));
    const float alpha = __builtin_amdgcn_exp2f((m - mx) * kScale);
    m = mx;
    l *= alpha;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] *= alpha;
#pragma unroll
    for (int b = 0; b < kBlocks; ++b) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float p = __builtin_amdgcn_exp2f((sc[b][reg] - m) * kScale);
        l += p;
        sc[b][reg] = p;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] = static_cast<__bf16>(sc[b][at::p_reg(u, j)]);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const bf16x4 lo = read_tr(at::v_read_index(kSplit, stage, wave, lane, b, u, db, 0));
          const bf16x4 hi = read_tr(at::v_read_index(kSplit, stage, wave, lane, b, u, db, 1));
          const bf16x8 vt = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, pb, o[db], 0, 0, 0);
        }
      }
    }

    if (kStages == 1) __syncthreads();   // the one stage has been read
    // with two, the other stage was last read before the barrier that ended tile kt - 1
    if (more) store_lds(kStages == 2 ? stage ^ 1 : 0);
    __syncthreads();
  }

  l += other_half(l);
  if (!kSplit) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = {o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(O + at::o_index(kSplit, head, qt, sq, wave, lane, db, g)) = v;
      }
  } else {
    // every wave is past the barrier that ended the last tile: the stages are free
    float* part = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = {o[db][4 * g], o[db][4 * g + 1], o[db][4 * g + 2], o[db][4 * g + 3]};
        *reinterpret_cast<f32x4*>(&part[at::merge_o_index(wave, lane & 31, at::o_col(lane, db, g))]) = v;
      }
    if (lane < 32) {
      part[at::merge_ml_index(wave, lane, 0)] = m;
      part[at::merge_ml_index(wave, lane, 1)] = l;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int query = at::merge_query(lane, i), d = at::merge_d(wave, lane);
      float top = part[at::merge_ml_index(0, query, 0)];
#pragma unroll
      for (int w = 1; w < 4; ++w) top = fmaxf(top, part[at::merge_ml_index(w, query, 0)]);
      float sum = 0.f;
      f32x4 acc = {};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float weight = __builtin_amdgcn_exp2f((part[at::merge_ml_index(w, query, 0)] - top) * kScale);
        sum += weight * part[at::merge_ml_index(w, query, 1)];
        acc += weight * *reinterpret_cast<const f32x4*>(&part[at::merge_o_index(w, query, d)]);
      }
      const float inv = 1.0f / sum;
      const size_t out = (at::query_row(kSplit, head, qt, sq, 0) + static_cast<size_t>(query)) * at::kD + static_cast<size_t>(d);
      *reinterpret_cast<f32x4*>(O + out) = acc * inv;
    }
  }
}

// ---------------------------------------------------------------------------- host

// Refused before any allocation or launch: a shape the tiles do not divide, and a launch or an iteration count
// that reaches HIP's 2^32 work-items.
void check_attn(const char* who, long long heads, long long sq, long long skv, long long iters) {
  if (!at::shape_ok(heads, sq, skv))
    throw std::invalid_argument(std::string(who) + ": heads is positive; sq is a positive multiple of 128 and skv of 64, or sq one of "
                                "32, 64, 96 and skv a positive multiple of 128; heads times the query tiles stays below 2^24 workgroups");
  if (iters <= 0 || static_cast<uint64_t>(iters) * at::kThreads >= gm::kWorkItemLimit)
    throw std::invalid_argument(std::string(who) + ": iterations in 1..2^24 - 1");
}

void attn_launch(hipStream_t s, const uint16_t* q, const uint16_t* k, const uint16_t* v, float* o, int heads, int sq, int skv) {
  const dim3 grid(static_cast<unsigned>(at::workgroups(heads, sq)));
  if (at::is_split(sq))
    hipLaunchKernelGGL(attn_bf16_kernel<true>, grid, dim3(at::kThreads), 0, s, q, k, v, o, sq, skv);
  else
    hipLaunchKernelGGL(attn_bf16_kernel<false>, grid, dim3(at::kThreads), 0, s, q, k, v, o, sq, skv);
}

double attn_tflops(int heads, int sq, int skv, int iters, double ms) {
  return at::flop(heads, sq, skv) * iters / (ms * 1e-3) / 1e12;
}

Tenant Tenant::attn(const std::vector<uint32_t>& mask, int heads, int sq, int skv, int iters) {
  Tenant t{Stream(mask), Events(), iters};
  t.kind = Kind::kAttn;
  t.attn_heads = heads, t.attn_sq = sq, t.attn_skv = skv;
  const size_t nq = static_cast<size_t>(heads) * sq * at::kD, nkv = static_cast<size_t>(heads) * skv * at::kD;
  t.ga = DevBuf<uint16_t>(nq, OomIsBadAlloc{});
  t.gb = DevBuf<uint16_t>(nkv, OomIsBadAlloc{});
  t.gv = DevBuf<uint16_t>(nkv, OomIsBadAlloc{});
  t.gc = DevBuf<float>(nq, OomIsBadAlloc{});
  gemm_fill(t.st.s, t.ga.p, nq, 0xa11ce5edu);
  gemm_fill(t.st.s, t.gb.p, nkv, 0xb0b5eedu);
  gemm_fill(t.st.s, t.gv.p, nkv, 0xca11ab1eu);
  return t;
}

// The numerics entry: small shapes only, so that it cannot serve as a burn.
std::vector<float> attn_bf16(const std::vector<float>& q, const std::vector<float>& k, const std::vector<float>& v, int heads, int sq,
                             int skv, int dev) {
  check_attn("attn_bf16", heads, sq, skv, 1);
  if (heads > 8 || sq > 512 || skv > 1024) throw std::invalid_argument("attn_bf16: heads at most 8, sq 512 and skv 1024");
  const size_t nq = static_cast<size_t>(heads) * sq * at::kD, nkv = static_cast<size_t>(heads) * skv * at::kD;
  if (q.size() != nq || k.size() != nkv || v.size() != nkv)
    throw std::invalid_argument("attn_bf16: q holds heads x sq x 128 values, k and v heads x skv x 128");
  HIP_OK(hipSetDevice(dev));
  std::vector<uint16_t> hq(nq), hk(nkv), hv(nkv);
  for (size_t i = 0; i < nq; ++i) hq[i] = st::f32_to_bf16_bits(q[i]);
  for (size_t i = 0; i < nkv; ++i) hk[i] = st::f32_to_bf16_bits(k[i]), hv[i] = st::f32_to_bf16_bits(v[i]);
  DevBuf<uint16_t> dq(nq), dk(nkv), dv(nkv);
  std::vector<float> o(nq);
  DevBuf<float> dout(nq);
  HIP_OK(hipMemcpy(dq.p, hq.data(), nq * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dk.p, hk.data(), nkv * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dv.p, hv.data(), nkv * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dout.p, 0xff, nq * 4));   // NaN wherever the kernel does not write
  attn_launch(nullptr, dq.p, dk.p, dv.p, dout.p, heads, sq, skv);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(o.data(), dout.p, nq * 4, hipMemcpyDeviceToHost));
  return o;
}

py::dict attn_throughput(int dev, const std::vector<uint32_t>& mask, int heads, int sq, int skv, int iters) {
  double ms = 0.0, tflops = 0.0;
  {
    py::gil_scoped_release nogil;
    check_attn("attn_throughput", heads, sq, skv, iters);
    HIP_OK(hipSetDevice(dev));
    std::vector<Tenant> tenants;
    tenants.push_back(Tenant::attn(mask, heads, sq, skv, iters));
    tflops = run_tenants(tenants)[0];
    ms = tenants[0].ev.ms();
  }
  py::dict d;
  d["ms"] = ms;
  d["tflops"] = tflops;
  d["gbs"] = at::compulsory_bytes(heads, sq, skv) * iters / (ms * 1e-3) / 1e9;
  d["heads"] = heads;
  d["sq"] = sq;
  d["skv"] = skv;
  d["iters"] = iters;
  d["kernel"] = at::is_split(sq) ? "split" : "wide";
  return d;
}

// The attention tenant on `attn_mask` next to an HBM copy on `hbm_mask`, as gemm_colocated: enqueued together, each
// timed by its own events, the caller sizing which outlasts the other. Returns {attention TFLOP/s, copy GB/s}.
std::vector<double> attn_colocated(int dev, const std::vector<uint32_t>& attn_mask, const std::vector<uint32_t>& hbm_mask,
                                   int heads, int sq, int skv, int attn_iters, size_t bytes, int hbm_iters) {
  check_attn("attn_colocated", heads, sq, skv, attn_iters);
  const size_t count = bytes / sizeof(float4);
  if (count == 0 || hbm_iters <= 0) throw std::invalid_argument("attn_colocated: bytes and hbm_iters must be positive");
  const unsigned grid = copy_grid(count);
  HIP_OK(hipSetDevice(dev));
  std::vector<Tenant> tenants;
  tenants.push_back(Tenant::attn(attn_mask, heads, sq, skv, attn_iters));
  tenants.push_back(Tenant::copy(hbm_mask, count, grid, hbm_iters));
  return run_tenants(tenants);
}
