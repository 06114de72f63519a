// The body of preprocess_backward_kernel and preprocess_backward_cam_kernel (rasterizer_backward.hip), included once in
// each: one source text, two kernels, so that the kernel without camera sums keeps its name, its arguments and its
// instruction stream.  Expects the kernels' parameters, `constexpr bool CAM` and `cam_out` in scope.
//
// NOT a translation unit of its own, and not a header to include anywhere else (the guard below stops that).
// With CAM no lane may leave the view loop early: the camera sums at the end of every view's iteration are DPP wave
// sums and need all 64 lanes, and the barrier after the loop needs all four waves.  A new `return` or `continue` in the
// body must be written as the existing ones are (`if (!CAM) continue;`, lanes without work fall through as `!live`).
#ifndef GR_PREPROCESS_BACKWARD_BODY_OK
#error "preprocess_backward_body.hpp is the body of the two preprocess backward kernels of rasterizer_backward.hip"
#endif
static_assert(std::is_same<decltype(CAM), const bool>::value, "the including kernel defines `constexpr bool CAM`");
  constexpr int NF = AUX ? NF_AUX : gr::NF;
  extern __shared__ float s_cam[];  // CAM: [V][4 waves][NCAM]
  const int i_raw = blockIdx.x * blockDim.x + threadIdx.x;
  if (!CAM && i_raw >= P) return;
  const bool active = !CAM || i_raw < P;
  const int i = active ? i_raw : 0;  // (a lane past P reads Gaussian 0 and writes nothing)
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const int K = (D + 1) * (D + 1);
  const float p[3] = {means3D[3 * (int64_t)i], means3D[3 * (int64_t)i + 1], means3D[3 * (int64_t)i + 2]};
  float sc[3] = {0.f, 0.f, 0.f}, rot[4] = {0.f, 0.f, 0.f, 0.f}, c6[6];
  if (HAS_COV) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * (int64_t)i + k];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) sc[k] = scales[3 * (int64_t)i + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) rot[k] = rotations[4 * (int64_t)i + k];
  }
  float shr[HAS_SH ? 48 : 1], dsh[HAS_SH ? 48 : 1];
  if (HAS_SH) {
#pragma unroll
    for (int k = 0; k < 48; ++k) {
      shr[k] = k < 3 * K ? shs[(int64_t)i * M * 3 + k] : 0.0f;
      dsh[k] = 0.0f;
    }
  }
  float dmean[3] = {0.f, 0.f, 0.f}, dcol[3] = {0.f, 0.f, 0.f}, dop = 0.f, dscale[3] = {0.f, 0.f, 0.f};
  float drot[4] = {0.f, 0.f, 0.f, 0.f}, dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int v = 0; v < V; ++v) {
    const int64_t o = (int64_t)v * P + i;
    const int64_t vbase = (int64_t)v * P;
    float* m2 = (out.means2D != nullptr && active) ? out.means2D + 3 * o : nullptr;
    int x0, y0, w, h;
    const uint32_t rr = rect_raw[o];
    const bool live = active && rr != 0u && rect_decode(rr, i, vbase, rec, gx, gy, x0, y0, w, h);
    float cf[NCAMF];  // (CAM only)
    if constexpr (CAM) {
#pragma unroll
      for (int k = 0; k < NCAMF; ++k) cf[k] = 0.0f;
    }
    if (!live) {
      if (m2) m2[0] = m2[1] = m2[2] = 0.0f;
      if (!CAM) continue;
    }
    if (live) {
      // this (view, Gaussian)'s slots, in rectangle order
      const int64_t s0 = (int64_t)slot_local[o] + block_pre[o >> 8];
      const int n = w * h;
      float gs[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) gs[f] = 0.0f;
      for (int k = 0; k < n; ++k) {
        if (s0 + k >= slot_cap) break;  // (never: see render_backward_kernel)
        const float* s = slots + NF * (s0 + k);
#pragma unroll
        for (int f = 0; f < NF; ++f) gs[f] += s[f];
      }
      const DevView& cam = views[v];
      // ---- forward quantities (same fp32 operations as preprocess_kernel)
      float pv[3], ph[4];
      xform4x3(cam.view, p, pv);
      xform4x4(cam.proj, p, ph);
      const float pw = 1.0f / (ph[3] + 0.0000001f);
      if (!HAS_COV) cov3d_from_scale_rot(sc, cam.scale_mod, rot, c6);
      const float tz = pv[2];
      const float limx = 1.3f * cam.tanx, limy = 1.3f * cam.tany;
      const float ux = pv[0] / tz, uy = pv[1] / tz;
      const float cux = fminf(limx, fmaxf(-limx, ux)), cuy = fminf(limy, fmaxf(-limy, uy));
      const float txp = cux * tz, typ = cuy * tz;
      const float J00 = cam.fx / tz, J02 = -(cam.fx * txp) / (tz * tz);
      const float J11 = cam.fy / tz, J12 = -(cam.fy * typ) / (tz * tz);
      const float* Vm = cam.view;
      float A0[3], A1[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        A0[j] = fmaf(J00, Vm[j * 4 + 0], J02 * Vm[j * 4 + 2]);
        A1[j] = fmaf(J11, Vm[j * 4 + 1], J12 * Vm[j * 4 + 2]);
      }
      const float S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
      float SA0[3], SA1[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        SA0[k] = fmaf(S[k][0], A0[0], fmaf(S[k][1], A0[1], S[k][2] * A0[2]));
        SA1[k] = fmaf(S[k][0], A1[0], fmaf(S[k][1], A1[1], S[k][2] * A1[2]));
      }
      const float a = fmaf(A0[0], SA0[0], fmaf(A0[1], SA0[1], A0[2] * SA0[2])) + 0.3f;
      const float b = fmaf(A1[0], SA0[0], fmaf(A1[1], SA0[1], A1[2] * SA0[2]));
      const float c = fmaf(A1[0], SA1[0], fmaf(A1[1], SA1[1], A1[2] * SA1[2])) + 0.3f;
      // ---- conic (c, -b, a) / det -> 2-D covariance
      const float det = a * c - b * b;
      const float inv2 = 1.0f / (det * det);
      const float gA = gs[2], gB = gs[3], gC = gs[4];
      const float ga = (-c * c * gA + b * c * gB - b * b * gC) * inv2;
      const float gb = (2.f * b * c * gA - (a * c + b * b) * gB + 2.f * a * b * gC) * inv2;
      const float gc = (-b * b * gA + a * b * gB - a * a * gC) * inv2;
      // ---- 2-D covariance = A S A^T -> 3-D covariance and A = J W
      float dc6[6];
      dc6[0] = A0[0] * A0[0] * ga + A1[0] * A0[0] * gb + A1[0] * A1[0] * gc;
      dc6[3] = A0[1] * A0[1] * ga + A1[1] * A0[1] * gb + A1[1] * A1[1] * gc;
      dc6[5] = A0[2] * A0[2] * ga + A1[2] * A0[2] * gb + A1[2] * A1[2] * gc;
      dc6[1] = 2.f * A0[0] * A0[1] * ga + (A1[0] * A0[1] + A1[1] * A0[0]) * gb + 2.f * A1[0] * A1[1] * gc;
      dc6[2] = 2.f * A0[0] * A0[2] * ga + (A1[0] * A0[2] + A1[2] * A0[0]) * gb + 2.f * A1[0] * A1[2] * gc;
      dc6[4] = 2.f * A0[1] * A0[2] * ga + (A1[1] * A0[2] + A1[2] * A0[1]) * gb + 2.f * A1[1] * A1[2] * gc;
      float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float gA0 = 2.f * ga * SA0[j] + gb * SA1[j];
        const float gA1 = gb * SA0[j] + 2.f * gc * SA1[j];
        dJ00 += gA0 * Vm[j * 4 + 0];
        dJ02 += gA0 * Vm[j * 4 + 2];
        dJ11 += gA1 * Vm[j * 4 + 1];
        dJ12 += gA1 * Vm[j * 4 + 2];
        if constexpr (CAM) {
          cf[6 + 3 * j] = gA0 * J00;
          cf[7 + 3 * j] = gA1 * J11;
          cf[8 + 3 * j] = gA0 * J02 + gA1 * J12;
        }
      }
      // J -> view-space mean t (the 1.3 tan(fov) clamp of x/z, y/z masks d/dt_x, d/dt_y where active)
      const float tz2 = tz * tz, tz3 = tz2 * tz;
      const float dtxp = -cam.fx / tz2 * dJ02, dtyp = -cam.fy / tz2 * dJ12;
      float dt[3];
      dt[2] = -cam.fx / tz2 * dJ00 - cam.fy / tz2 * dJ11 + 2.f * cam.fx * txp / tz3 * dJ02 +
              2.f * cam.fy * typ / tz3 * dJ12;
      const bool inx = ux >= -limx && ux <= limx, iny = uy >= -limy && uy <= limy;
      dt[0] = inx ? dtxp : 0.0f;
      dt[1] = iny ? dtyp : 0.0f;
      if (!inx) dt[2] += dtxp * cux;
      if (!iny) dt[2] += dtyp * cuy;
      // ---- NDC mean (means2D.grad: dL/dNDC, upstream's 0.5 W / 0.5 H factors) -> homogeneous projection
      const float dnx = gs[0] * (0.5f * (float)W), dny = gs[1] * (0.5f * (float)H);
      if (m2) m2[0] = dnx, m2[1] = dny, m2[2] = 0.0f;
      const float dph0 = dnx * pw, dph1 = dny * pw;
      const float dph3 = -(dnx * ph[0] + dny * ph[1]) * pw * pw;
      const float* Pm = cam.proj;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        dmean[j] += Pm[j * 4 + 0] * dph0 + Pm[j * 4 + 1] * dph1 + Pm[j * 4 + 3] * dph3 +
                    Vm[j * 4 + 0] * dt[0] + Vm[j * 4 + 1] * dt[1] + Vm[j * 4 + 2] * dt[2];
      if constexpr (AUX) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dmean[j] += gs[9] * Vm[j * 4 + 2];
      }
      if constexpr (CAM) {
        cf[0] = dph0, cf[1] = dph1, cf[2] = dph3;
        cf[3] = dt[0], cf[4] = dt[1], cf[5] = dt[2];
        if constexpr (AUX) cf[5] += gs[9];
      }
      dop += gs[5];
      // ---- colour
      if (HAS_SH) {
        float rgb[3];
        sh_to_rgb(D, p, cam.campos, [&](int k, int ch) { return shr[k * 3 + ch]; }, rgb);  // the forward's clamp decision
        const float d0 = p[0] - cam.campos[0], d1 = p[1] - cam.campos[1], d2 = p[2] - cam.campos[2];
        const float len = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
        const float x = d0 / len, y = d1 / len, z = d2 / len;
        float B[16], Bx[16], By[16], Bz[16];
        sh_basis_grad(D, x, y, z, B, Bx, By, Bz);
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float gcol = rgb[ch] > 0.0f ? gs[6 + ch] : 0.0f;
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            dsh[k * 3 + ch] += B[k] * gcol;
            ddx += Bx[k] * shr[k * 3 + ch] * gcol;
            ddy += By[k] * shr[k * 3 + ch] * gcol;
            ddz += Bz[k] * shr[k * 3 + ch] * gcol;
          }
        }
        const float dot = x * ddx + y * ddy + z * ddz;
        dmean[0] += (ddx - x * dot) / len;
        dmean[1] += (ddy - y * dot) / len;
        dmean[2] += (ddz - z * dot) / len;
        if constexpr (CAM) {
          cf[15] = -((ddx - x * dot) / len);
          cf[16] = -((ddy - y * dot) / len);
          cf[17] = -((ddz - z * dot) / len);
        }
      } else {
        dcol[0] += gs[6];
        dcol[1] += gs[7];
        dcol[2] += gs[8];
      }
      // ---- 3-D covariance
      if (HAS_COV) {
#pragma unroll
        for (int k = 0; k < 6; ++k) dcov[k] += dc6[k];
      } else {
        const float mod = cam.scale_mod;
        const float s[3] = {mod * sc[0], mod * sc[1], mod * sc[2]};
        const float r = rot[0], x = rot[1], y = rot[2], z = rot[3];
        float R[3][3];
        R[0][0] = 1.f - 2.f * (y * y + z * z);
        R[0][1] = 2.f * (x * y - r * z);
        R[0][2] = 2.f * (x * z + r * y);
        R[1][0] = 2.f * (x * y + r * z);
        R[1][1] = 1.f - 2.f * (x * x + z * z);
        R[1][2] = 2.f * (y * z - r * x);
        R[2][0] = 2.f * (x * z - r * y);
        R[2][1] = 2.f * (y * z + r * x);
        R[2][2] = 1.f - 2.f * (x * x + y * y);
        // Sigma = Mt^T Mt with Mt[k][i] = s_k R[i][k]; symmetric upstream gradient Gs (off-diagonals carry half of dc6)
        const float Gs[3][3] = {{dc6[0], 0.5f * dc6[1], 0.5f * dc6[2]},
                                {0.5f * dc6[1], dc6[3], 0.5f * dc6[4]},
                                {0.5f * dc6[2], 0.5f * dc6[4], dc6[5]}};
        float dR[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float ds = 0.f;
#pragma unroll
          for (int ii = 0; ii < 3; ++ii) {
            float dM = 0.f;  // dL/dMt[k][ii] = 2 sum_j Mt[k][j] Gs[j][ii]
#pragma unroll
            for (int j = 0; j < 3; ++j) dM += s[k] * R[j][k] * Gs[j][ii];
            dM *= 2.f;
            ds += dM * R[ii][k];
            dR[ii][k] = s[k] * dM;
          }
          dscale[k] += mod * ds;
        }
        drot[0] += 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
        drot[1] += 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] +
                          r * dR[2][1] - 2.f * x * dR[2][2]);
        drot[2] += 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] +
                          z * dR[2][1] - 2.f * y * dR[2][2]);
        drot[3] += 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] +
                          y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
      }
    }  // live
    if constexpr (CAM) {
      // all 64 lanes are here; lane f keeps sum f, one LDS write per (view, wave)
      const int lane = threadIdx.x & (WAVE - 1);
      float mine = 0.0f;
      if (__ballot(live) != 0ull) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pj = !live ? 0.0f : (j < 3 ? p[j % 3] : 1.0f);  // (0: a culled mean may be anything)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float sv = wave_sum_f32_dpp(j < 3 ? pj * cf[3 + c] + cf[6 + 3 * (j % 3) + c] : pj * cf[3 + c]);
            if (lane == 3 * j + c) mine = sv;
            const float sp = wave_sum_f32_dpp(pj * cf[c]);
            if (lane == 12 + 3 * j + c) mine = sp;
          }
        }
        if (HAS_SH) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float sc3 = wave_sum_f32_dpp(cf[15 + c]);
            if (lane == 24 + c) mine = sc3;
          }
        }
      }
      if (lane < NCAM) s_cam[(v * 4 + (int)(threadIdx.x / WAVE)) * NCAM + lane] = mine;
    }
  }
  if constexpr (CAM) {
    __syncthreads();
    // the four waves in order -> this workgroup's partial of every view
    for (int k = threadIdx.x; k < V * NCAM; k += 256) {
      const int v = k / NCAM, f = k - v * NCAM;
      const float* s = s_cam + v * 4 * NCAM + f;
      cam_out.partial[((int64_t)v * gridDim.x + blockIdx.x) * NCAM + f] = ((s[0] + s[NCAM]) + s[2 * NCAM]) + s[3 * NCAM];
    }
    if (!active) return;
  }
  if (out.means3D)
    for (int k = 0; k < 3; ++k) out.means3D[3 * (int64_t)i + k] = dmean[k];
  if (out.opacity) out.opacity[i] = dop;
  if (HAS_SH && out.shs) {
    float* dst = out.shs + (int64_t)i * M * 3;
#pragma unroll
    for (int k = 0; k < 48; ++k)
      if (k < 3 * M) dst[k] = dsh[k];
    for (int k = 48; k < 3 * M; ++k) dst[k] = 0.0f;  // coefficients past degree 3
  }
  if (!HAS_SH && out.colors)
    for (int k = 0; k < 3; ++k) out.colors[3 * (int64_t)i + k] = dcol[k];
  if (HAS_COV && out.cov3D)
    for (int k = 0; k < 6; ++k) out.cov3D[6 * (int64_t)i + k] = dcov[k];
  if (!HAS_COV) {
    if (out.scales)
      for (int k = 0; k < 3; ++k) out.scales[3 * (int64_t)i + k] = dscale[k];
    if (out.rotations)
      for (int k = 0; k < 4; ++k) out.rotations[4 * (int64_t)i + k] = drot[k];
  }
