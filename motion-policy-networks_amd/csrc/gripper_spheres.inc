// gripper_spheres.inc -- the gripper's rows of the sphere table (links 9, 12, 13), in table order, as points of the
// right_gripper frame, compacted into LDS: a point h of the hand frame sits at (-h_x, -h_y, h_z - 0.1); a fingertip frame is
// the hand frame shifted by (0, +-finger, 0.0584 + 0.045).  Wave 1 lane s takes row s (S <= 64).  Included as a statement
// block by gripper_roadmap.hip, gripper_roadmap_cloud.hip, task_candidates.hip and the two gripper shortcut kernels
// (gripper_shortcut.hip, gripper_shortcut_cloud.hip); the compiler sees the lines it saw when the first wrote them
// out (profiles/gripper_roadmap_cloud_timing.md has the instruction-stream comparison).
//   in scope: k (the wave), lane, sc, sr, sl, S, finger, float *gsph (GRM_MAX_SPHERES x 4: point, radius), int *ng_lds
//   The caller's barrier publishes the rows and the count.
if (k == 1) {
  const int link = lane < S ? sl[lane] : -1;
  const bool mine_g = link == 9 || link == 12 || link == 13;
  const unsigned long long gmask = __builtin_amdgcn_ballot_w64(mine_g);
  if (mine_g) {
    float *dst = gsph + 4 * __builtin_popcountll(gmask & (((unsigned long long)1 << lane) - 1));
    const float hy = link == 12 ? sc[3 * lane + 1] + finger : link == 13 ? sc[3 * lane + 1] - finger : sc[3 * lane + 1];
    const float hz = link == 9 ? sc[3 * lane + 2] : sc[3 * lane + 2] + (0.0584f + 0.045f);
    dst[0] = -sc[3 * lane + 0], dst[1] = -hy, dst[2] = hz - 0.1f, dst[3] = sr[lane];
  }
  if (lane == 0) *ng_lds = __builtin_popcountll(gmask);
}
