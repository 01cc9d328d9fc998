// franka_live_rows.inc -- problem b's live primitives, compacted into 128 LDS rows of 16 floats,
// [R | Rt (3 x 4 floats) | full sizes]: cuboids from row 0, cylinders from row 64 (M1, M2 <= 64).  Lane m of a wave tests
// primitive m; a live one takes the slot = number of live ones before it.  Included as a statement block by ik.hip,
// plan.hip, roadmap.hip, gripper_roadmap.hip, gripper_shortcut.hip and task_candidates.hip (one inline function for both made franka_ik_kernel slower: profiles/franka_device_timing.md); the compiler
// sees the lines it saw when each kernel wrote them out.
//   in scope: b, lane, cub_f, cub_d, M1, cyl_f, cyl_r, cyl_h, M2, float *prim_rows
//   FRANKA_LIVE_ROWS_STORE: this wave writes the rows (every wave gets the counts)
//   defines:  n_cub, n_cyl.  The caller's barrier publishes the rows.
// franka_collision_env_kernel stages rows of another format (half sizes, float4, the last waves) and keeps its own form.
const float *cf = cub_f + (size_t)b * M1 * 16;
const float *cd = cub_d + (size_t)b * M1 * 3;
const float *yf = cyl_f + (size_t)b * M2 * 16;
const float *yr = cyl_r + (size_t)b * M2;
const float *yh = cyl_h + (size_t)b * M2;
bool clive = false, ylive = false;
float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, r0 = 0.0f, h0 = 0.0f;
if (lane < M1) {
  c0 = cd[3 * lane + 0], c1 = cd[3 * lane + 1], c2 = cd[3 * lane + 2];
  clive = !(mpx_is_zero(c0) || mpx_is_zero(c1) || mpx_is_zero(c2));
}
if (lane < M2) {
  r0 = yr[lane], h0 = yh[lane];
  ylive = !(mpx_is_zero(r0) || mpx_is_zero(h0));
}
const unsigned long long cmask = __builtin_amdgcn_ballot_w64(clive), ymask = __builtin_amdgcn_ballot_w64(ylive);
const int n_cub = __builtin_popcountll(cmask), n_cyl = __builtin_popcountll(ymask);
const unsigned long long below = ((unsigned long long)1 << lane) - 1;
if ((FRANKA_LIVE_ROWS_STORE) && clive) {
  float *dst = prim_rows + 16 * __builtin_popcountll(cmask & below);
#pragma unroll
  for (int i = 0; i < 12; ++i) dst[i] = cf[16 * lane + i];
  dst[12] = c0, dst[13] = c1, dst[14] = c2;
}
if ((FRANKA_LIVE_ROWS_STORE) && ylive) {
  float *dst = prim_rows + 16 * (64 + __builtin_popcountll(ymask & below));
#pragma unroll
  for (int i = 0; i < 12; ++i) dst[i] = yf[16 * lane + i];
  dst[12] = r0, dst[13] = h0;
}
