"""CPU: csrc/launch_routes.h stands alone -- a stand-alone C++17 program that includes nothing else compiles with a host
compiler (no HIP), walks every route function over wide grids of shapes under the undefined-behaviour sanitizer without a
report, and on a handful of shapes prints exactly what the library's route queries answer."""
import os
import shutil
import subprocess

import pytest

import launch_routes as lr

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "motion-policy-networks_amd", "csrc")
# kind -> (the header's function, its fields in the query's order, the library's query)
KINDS = {"fps": ("fps_route", "family pts threads lds", "mpx_fps_route"),
         "col": ("collision_route", "form ppt block tc chunks last", "mpx_franka_collision_route"),
         "lin": ("linear_route", "form S kslice", "mpx_linear_route"),
         "wg": ("wgrad_route", "tile splits rows_per_split", "mpx_linear_wgrad_route"),
         "sa": ("sa_route", "packed Q lpool units epx persistent slots resident one_env xcd_aware", "mpx_sa_mlp_route")}
# the shapes printed and compared with the library: (kind, arguments of the header's function)
SHAPES = ([("fps", (B, N, f)) for B in (2, 767, 768) for N in (1, 512, 513, 4096, 4097, 6272, 8192) for f in (0, 1)]
          + [("col", a) for a in ((3, 1, 56, 16, 16, 1), (2, 62, 57, 16, 16, 1), (3, 130, 56, 40, 16, 1), (3, 66, 16, 16, 16, 1),
                                  (3, 9, 56, 70, 16, 1), (3, 50, 56, 16, 16, 0), (0, 5, 56, 16, 16, 1))]
          + [(k, (M, N, K)) for k in ("lin", "wg") for M in (1, 4, 10, 256, 1025, 1048576) for N, K in ((4096, 1024), (512, 2112), (128, 68), (64, 4))]
          + [("sa", (cus, B, np_, 128, cnt, C, x3, fac, 1)) for cus in (8, 256, 304) for B in (1, 4, 256, 1027, 8192)
             for np_, C, fac in ((512, 1, 0), (128, 64, 1)) for x3 in (0, 1) for cnt in (0, 1) if cnt or not fac])
POOL_SHAPES = [(Q, C, K) for Q in (1, 10, 512, 4194304) for C, K in ((64, 64), (256, 128), (1024, 512))]

MAIN = r"""
#include "launch_routes.h"
#include <stdio.h>
int main() {  // the grids: every size at which a launcher's choice can change, and the model's layers
  const int Bf[] = {1, 2, 767, 768, 8192}, Ss[] = {1, 16, 24, 32, 33, 40, 48, 56, 57, 64, 65}, Ms[][2] = {{16, 16}, {64, 64}, {65, 16}, {16, 65}};
  const int Mr[] = {1, 2, 3, 4, 5, 8, 9, 10, 128, 256, 1024, 1025, 4096, 1048576}, Bs[] = {1, 2, 4, 8, 255, 256, 1027, 8192}, Cu[] = {8, 256, 304};
  const int NK[][2] = {{4096, 1024}, {2048, 4096}, {1024, 2048}, {32, 8}, {64, 32}, {128, 64}, {128, 128}, {64, 128}, {512, 2112}, {256, 512},
                       {128, 256}, {8, 128}, {64, 4}, {64, 64}, {128, 68}, {256, 128}, {256, 260}, {512, 256}, {1024, 512}};
  const long long Qs[] = {1, 4, 8, 10, 256, 512, 131072, 4194304};
  long long sum = 0;
  for (int B : Bf) for (int N = 1; N <= FPS_MAX_N; ++N) for (int f = 0; f < 2; ++f) sum += fps_route(B, N, f).pts + opt_n_threads_log2(N);
  for (int T = 1; T <= 200; ++T) for (int S : Ss) for (auto &m : Ms) for (int al = 0; al < 2; ++al) for (int B = 0; B < 4; ++B)
    sum += collision_route(B, T, S, m[0], m[1], al != 0).last;
  for (int M : Mr) for (auto &nk : NK) for (int sw = 0; sw < 2; ++sw) sum += linear_route(M, nk[sw], nk[1 - sw]).kslice + wgrad_route(M, nk[sw], nk[1 - sw]).rows_per_split;
  for (long long Q : Qs) for (auto &nk : NK) sum += pool_wgrad_splits(Q, nk[0], nk[1]);
  for (int B : Bs) for (int cus : Cu) for (int x3 = 0; x3 < 2; ++x3) for (int cnt = 0; cnt < 2; ++cnt)
    sum += sa_route(cus, B, 512, 128, cnt != 0, 1, x3 != 0, false, true).units + sa_route(cus, B, 128, 128, true, 64, x3 != 0, true, true).units;
  printf("walked %lld\n", sum);
%s
  return 0;
}
"""


def test_header_stands_alone_and_the_library_answers_the_same(tmp_path):
    from mpinets_amd import _lib

    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    prints = ['{ const auto r = %s(%s); printf("%s\\n", %s); }' % (
        KINDS[k][0], ", ".join(map(str, args)), " ".join(["%d"] * len(KINDS[k][1].split())),
        ", ".join("(int)r." + f for f in KINDS[k][1].split())) for k, args in SHAPES]
    prints += ['printf("%%d\\n", (int)pool_wgrad_splits(%d, %d, %d));' % a for a in POOL_SHAPES]
    src, exe = tmp_path / "routes_main.cpp", tmp_path / "routes_main"
    src.write_text(MAIN.replace("%s", "\n".join("  " + p for p in prints)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I",
                           HEADER_DIR, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert lines[0].startswith("walked ") and len(lines) == 1 + len(SHAPES) + len(POOL_SHAPES)
    lib = _lib.load()
    for (kind, args), line in zip(SHAPES + [("pool", a) for a in POOL_SHAPES], lines[1:]):
        want = [int(v) for v in line.split()]
        if kind == "fps":
            assert lr.fps_fields(*args) == want, (args, line)
        else:
            name = "mpx_pool_wgrad_route" if kind == "pool" else KINDS[kind][2]
            assert lr._query(name, len(want), *args) == want, (kind, args, line)
    assert lib.mpx_get_variant(lr.MPX_VARIANT_FPS) == 1
