// The body of preprocess_kernel and preprocess_many_kernel (rasterizer.hip), included once in each: one source text, two
// kernels, so that the kernel for up to four views per call keeps its name, its arguments and its instruction stream.
// Expects the kernels' parameters and `constexpr bool WAVE_MM` in scope.
//   WAVE_MM  (more than four views per call, bucket depth sort behind it): key_mm gets the key range of every WAVE
//            ([V][4 * blocks]; never null) -- no barrier in the view loop; a launch of the sort reduces a view's row
//            (depth_sort.hip, ds_range_kernel).
// NOT a translation unit of its own, and not a header to include anywhere else (the guard below stops that).
#ifndef GR_PREPROCESS_BODY_OK
#error "preprocess_body.hpp is the body of the two preprocess kernels of rasterizer.hip"
#endif
static_assert(std::is_same<decltype(WAVE_MM), const bool>::value, "the including kernel defines `constexpr bool WAVE_MM`");
  // LATE (one camera per call): the camera arrives in the kernel arguments `cam1` (no upload in front of the frame); the first
  // block leaves it in `views` for the kernels behind this one.  far_seq: the value a far depth stores into *far_flag
  // (a per-call stamp when nobody cleared the flag, else 1).
  if (LATE && blockIdx.x == 0 && threadIdx.x < (int)(sizeof(DevView) / 4))
    reinterpret_cast<float*>(const_cast<DevView*>(views))[threadIdx.x] = reinterpret_cast<const float*>(&cam1)[threadIdx.x];
  __shared__ float4 s_sh[(SH16 && !LATE) ? WAVE * SH_ROW : 1];
  __shared__ float4 s_rec[256 / WAVE][4 * REC_PLANE];
  __shared__ int s_mm[WAVE_MM ? 1 : 2][2][256 / WAVE];  // [view parity][min, max][wave]
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  float shr[SH16 ? 48 : 1];
  if (SH16 && !LATE) {
    // degree-3 SH = 192 B per Gaussian: the block's 48 KB are read as a coalesced float4 stream and transposed through
    // LDS (row stride 13 float4 keeps the per-thread ds_read_b128 conflict-free), one wave's 64 Gaussians at a time through
    // the same 13 KB -- a 52 KB staging area for all four waves capped the CU at 12 resident waves for the whole view loop.
    const int g0 = blockIdx.x * 256;
    const int n_here = min(256, P - g0);
    const float4* src = reinterpret_cast<const float4*>(shs + (int64_t)g0 * 48);
#pragma unroll 1
    for (int w = 0; w < 256 / WAVE; ++w) {
      const int lim = min(WAVE, n_here - w * WAVE) * 12;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int f = threadIdx.x + u * 256;
        if (f < lim) {
          const int g = f / 12, j = f - g * 12;
          s_sh[g * SH_ROW + j] = src[w * WAVE * 12 + f];
        }
      }
      __syncthreads();
      if ((int)threadIdx.x / WAVE == w && i < P) {
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          const float4 t = s_sh[(threadIdx.x & (WAVE - 1)) * SH_ROW + j];
          shr[4 * j] = t.x;
          shr[4 * j + 1] = t.y;
          shr[4 * j + 2] = t.z;
          shr[4 * j + 3] = t.w;
        }
      }
      __syncthreads();
    }
  }
  // Threads past the end stay alive (they help to write their wave's records below) on a clamped index and store nothing.
  const bool valid = i < P;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_first = i - lane;  // first Gaussian of this wave
  i = min(i, P - 1);
  const float p[3] = {means3D[3 * (int64_t)i], means3D[3 * (int64_t)i + 1], means3D[3 * (int64_t)i + 2]};
  const float opacity = opacities[i];
  float c6[6];
  if (HAS_COV) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * (int64_t)i + k];
  }
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const float* sh = HAS_SH ? shs + (int64_t)i * M * 3 : nullptr;
  float cpre[3] = {0.f, 0.f, 0.f};
  if (!HAS_SH) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cpre[k] = colors_precomp[3 * (int64_t)i + k];
  }
  float4* wrec = s_rec[threadIdx.x / WAVE];
  float mod_prev = 0.f;
  bool have_cov = HAS_COV;
  for (int v = 0; v < V; ++v) {
    const DevView& cam = LATE ? cam1 : views[v];
    const int64_t o = (int64_t)v * P + i;
    int out_radius = 0;
    uint32_t out_field = 0u, out_rect = 0u;  // culled: depth field 0
    float out_depth = 0.f, out_sxx = INFINITY, out_syy = INFINITY, out_kc = 0.f;
    float2 out_xy = make_float2(0.f, 0.f);
    float4 out_co = make_float4(0.f, 0.f, 0.f, 0.f);
    bool shade = false;
    float rgb[3] = {0.f, 0.f, 0.f};
    float pv[3];
    xform4x3(cam.view, p, pv);
    if (pv[2] > 0.2f) {
      float ph[4];
      xform4x4(cam.proj, p, ph);
      const float pw = 1.0f / (ph[3] + 0.0000001f);
      const float pprojx = ph[0] * pw, pprojy = ph[1] * pw;
      if (!HAS_COV && (!have_cov || cam.scale_mod != mod_prev)) {
        // scales / rotations are read again here rather than held across the view loop: cov3D changes only with scale_mod
        float sc[3], rot[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) sc[k] = scales[3 * (int64_t)i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) rot[k] = rotations[4 * (int64_t)i + k];
        cov3d_from_scale_rot(sc, cam.scale_mod, rot, c6);
        have_cov = true;
        mod_prev = cam.scale_mod;
      }
      float cv[3];
      cov2d(pv, cam.fx, cam.fy, cam.tanx, cam.tany, c6, cam.view, cv);
      const float det = cv[0] * cv[2] - cv[1] * cv[1];
      if (det != 0.0f) {
        const float det_inv = 1.f / det;
        const float mid = 0.5f * (cv[0] + cv[2]);
        const float sq = sqrtf(fmaxf(0.1f, mid * mid - det));
        const float l1 = mid + sq, l2 = mid - sq;
        const float my_radius = ceilf(3.f * sqrtf(fmaxf(l1, l2)));
        const float px = ((pprojx + 1.0f) * (float)W - 1.0f) * 0.5f;
        const float py = ((pprojy + 1.0f) * (float)H - 1.0f) * 0.5f;
        int rmin[2], rmax[2];
        get_rect(px, py, (int)my_radius, gx, gy, rmin, rmax);
        const int ntile = (rmax[0] - rmin[0]) * (rmax[1] - rmin[1]);
        if (ntile != 0) {
          shade = true;
          if (HAS_SH && SH16 && LATE) {
            // one camera: the coefficients are loaded here and used at once -- ahead of this view's stores, which a load
            // issued after them would wait for
            const float4* s4 = reinterpret_cast<const float4*>(shs + (int64_t)i * 48);
#pragma unroll
            for (int jj = 0; jj < 12; ++jj) {
              const float4 t4 = s4[jj];
              shr[4 * jj] = t4.x;
              shr[4 * jj + 1] = t4.y;
              shr[4 * jj + 2] = t4.z;
              shr[4 * jj + 3] = t4.w;
            }
            sh_to_rgb(D, p, cam.campos, [&](int k, int c) { return shr[k * 3 + c]; }, rgb);
          }
          out_depth = pv[2];
          out_radius = (int)my_radius;
          out_xy = make_float2(px, py);
          out_co = make_float4(cv[2] * det_inv, -cv[1] * det_inv, cv[0] * det_inv, opacity);
          // kc: k such that |d|^2 > |pc| * k  ==>  fp32 power < pc for any cutoff pc < 0 (blend
          // cell culling).  power <= -|d|^2 (0.5/l1 - 2e-6): the 2e-6 covers the fp32 evaluation
          // error of the quadratic form given lambda_min(cov) >= 0.3 (the +0.3 dilation).
          const bool cullable = det > 0.0f && l2 >= 0.29f && l1 < 1.0e4f;
          const float kc = cullable ? 1.001f / (0.5f / l1 - 2.0e-6f) : INFINITY;
          out_kc = kc;
          // Tile rectangle actually emitted: the reference square (radius = ceil(3 sigma_max)) intersected with the
          // bounding box of the region where alpha can reach 1/255.  A pixel contributes only if fp32 power >= pc
          // (pc as in the blend, with margin); inside the cutoff circle rc2 the fp32 quadratic form is within
          // 2e-6 rc2 of the exact one, whose level set {0.5 d^T A d <= c'} has half-extents sqrt(2 c' Sigma_xx / yy).
          // Only (tile, Gaussian) pairs that blend nothing are dropped, so the image is unchanged; `radii` is not.
          if (cullable) {
            // blend cell culling along the axes: |dx|^2 > c' * sxx (or |dy|^2 > c' * syy) ==> no contribution
            out_sxx = 2.0f * cv[0] * 1.004f;
            out_syy = 2.0f * cv[2] * 1.004f;
            const float pcm = __logf(255.0f * opacity) + 2.0e-3f;
            if (pcm > 0.0f) {
              const float cp = pcm + 2.0e-6f * (pcm * kc);
              const float hx = sqrtf(2.0f * cp * cv[0]) * 1.001f + 1.0e-2f;
              const float hy = sqrtf(2.0f * cp * cv[2]) * 1.001f + 1.0e-2f;
              // pixels x with |x - px| <= hx: [ceil(px - hx), floor(px + hx)] -> tiles
              const float xlo = ceilf(px - hx), xhi = floorf(px + hx), ylo = ceilf(py - hy), yhi = floorf(py + hy);
              if (xlo > -1.0e6f && xhi < 1.0e6f && ylo > -1.0e6f && yhi < 1.0e6f) {
                rmin[0] = max(rmin[0], (int)floorf(xlo / (float)TILE));
                rmin[1] = max(rmin[1], (int)floorf(ylo / (float)TILE));
                rmax[0] = min(rmax[0], (int)floorf(xhi / (float)TILE) + 1);
                rmax[1] = min(rmax[1], (int)floorf(yhi / (float)TILE) + 1);
                if (rmax[0] < rmin[0]) rmax[0] = rmin[0];
                if (rmax[1] < rmin[1]) rmax[1] = rmin[1];
              }
            }
          }
          uint32_t dk = __float_as_uint(out_depth) - KEY_DEPTH_BASE;  // out_depth > 0.2 > 0.125
          if (dk >= (1u << KEY_DEPTH_BITS)) {
            dk = (1u << KEY_DEPTH_BITS) - 1;
            if (LATE) *far_flag = far_seq; else atomicOr(far_flag, 1);
          }
          out_field = dk;
          out_rect = pack_rect(rmin, rmax);
        }
      }
    }
    if (valid) {
      __builtin_nontemporal_store(out_radius, radii + o);  // (an output nobody in the pipeline reads)
      dfield[o] = out_field;
      rect_raw[o] = out_rect;
    }
    // Record pieces 0, 1 and 3 go to LDS before the colour is evaluated: the SH coefficients are the largest live set of
    // the loop, and no other record value is held in registers beside them.
    wrec[0 * REC_PLANE + lane] = make_float4(out_xy.x, out_xy.y, out_sxx, out_syy);
    wrec[1 * REC_PLANE + lane] = out_co;
    wrec[3 * REC_PLANE + lane] = make_float4(__int_as_float(out_radius), out_depth, 0.f, 0.f);  // wide-rectangle fallback only
    if (WAVE_MM) {
      // the wave's key range of this view: one 8-byte store of lane 0, nothing shared with the other waves
      const uint32_t fld = valid ? out_field : 0u;
      const int mn = wave_min_i32_dpp(fld != 0u ? (int)fld : 0x7fffffff), mx = wave_max_i32_dpp((int)fld);
      const int wave_id = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE));
      if (lane == 0) key_mm[(int64_t)v * (gridDim.x * (256 / WAVE)) + wave_id] = make_int2(mn, mx);
      // (nothing moves across this point, as across the barrier of the other kernel -- wave scope: no instruction.  Free to
      // move code the compiler ends at 130 registers for the 16-coefficient instances, a wave per SIMD less)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else if (key_mm != nullptr) {  // the block's key range of this view, for the bucket sort (depth_sort.hip)
      const uint32_t fld = valid ? out_field : 0u;
      const int mn = wave_min_i32_dpp(fld != 0u ? (int)fld : 0x7fffffff), mx = wave_max_i32_dpp((int)fld);
      if (lane == 0) s_mm[v & 1][0][threadIdx.x / WAVE] = mn, s_mm[v & 1][1][threadIdx.x / WAVE] = mx;
      __syncthreads();  // (one barrier per view: the other half of s_mm is the one the next view writes)
      if (threadIdx.x == 0) {
        int bmn = 0x7fffffff, bmx = 0;
#pragma unroll
        for (int w = 0; w < 256 / WAVE; ++w) bmn = min(bmn, s_mm[v & 1][0][w]), bmx = max(bmx, s_mm[v & 1][1][w]);
        key_mm[(int64_t)v * gridDim.x + blockIdx.x] = make_int2(bmn, bmx);
      }
    }
    if (shade && !(HAS_SH && SH16 && LATE)) {
      if (HAS_SH) {
        if (SH16) sh_to_rgb(D, p, cam.campos, [&](int k, int c) { return shr[k * 3 + c]; }, rgb);
        else sh_to_rgb(D, p, cam.campos, [&](int k, int c) { return sh[k * 3 + c]; }, rgb);
      } else {
        rgb[0] = cpre[0]; rgb[1] = cpre[1]; rgb[2] = cpre[2];
      }
    }
    wrec[2 * REC_PLANE + lane] = make_float4(rgb[0], rgb[1], rgb[2], out_kc);
    // The wave's 64 records (4 KB, contiguous) leave through LDS: lane l stores piece l % 4 of record 16 k + l / 4 in
    // store k, so every store instruction covers whole lines.  (Each lane writing its own record piece by piece costs four
    // partial-line writes per record: measured 0.26 ms of the 0.77 ms kernel at 32 views.)  Culled Gaussians are never
    // gathered: their 64-B line is not touched at all.
    const unsigned long long vis = __ballot(valid && out_radius > 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float4* wout = rec + 4 * ((int64_t)v * P + wave_first);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rl = 16 * k + lane / 4;
      const float4 piece = wrec[(lane & 3) * REC_PLANE + rl];
      // streaming stores (whole 64-byte records, 1 KB per instruction): the records are next read by the blend, three
      // stages later and in another order -- kept out of the caches they no longer evict the depth fields and rectangles the
      // sort is about to read (32 views: preprocess 0.61 -> 0.56 ms, depth sort 0.46 -> 0.41 ms)
      if ((vis >> rl) & 1ull) {
        typedef float pre_f4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(pre_f4{piece.x, piece.y, piece.z, piece.w}, reinterpret_cast<pre_f4*>(wout + 4 * rl + (lane & 3)));
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
