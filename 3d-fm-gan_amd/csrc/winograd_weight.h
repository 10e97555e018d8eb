// U = G g Gt of one 3x3 filter, G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]: the one statement of the Winograd F(2x2,3x3) weight
// transform, shared by wino_weight_f32 (winograd.hip) and the live-weight refresh (live_weights.hip) so that both give the
// same bits.  Two adds and an exact product by 0.5 per stage; nothing here can contract into an fma.
#pragma once

__device__ __forceinline__ void wino_weight_transform(const float (&g)[3][3], float (&u)[16]) {
  float tmp[4][3];      // G g
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    tmp[0][k] = g[0][k];
    tmp[1][k] = 0.5f * (g[0][k] + g[1][k] + g[2][k]);
    tmp[2][k] = 0.5f * (g[0][k] - g[1][k] + g[2][k]);
    tmp[3][k] = g[2][k];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    u[a * 4 + 0] = tmp[a][0];
    u[a * 4 + 1] = 0.5f * (tmp[a][0] + tmp[a][1] + tmp[a][2]);
    u[a * 4 + 2] = 0.5f * (tmp[a][0] - tmp[a][1] + tmp[a][2]);
    u[a * 4 + 3] = tmp[a][2];
  }
}
