"""CPU: static checks on the gfx950 code objects inside the built ``libmpinets_hip.so``.

Some kernels wait for their DMA loads with hard-coded ``vmcnt`` counts (``sa3_front_bf16x3_kernel``'s ``open_chunk`` in
csrc/sa3_front_bf16.hip, ``linear_bf16x3_pairs_kernel``'s ``WAIT_ONE`` in csrc/dense_bf16.hip).  Such a count is right
only while the compiler emits exactly the vector-memory operations the source expects.  A register spill adds scratch
loads / stores to the same counter, the wait then returns before the LDS data has landed, and the activations come out
silently wrong.  So those kernels must have no scratch at all: private segment 0 and no VGPR / SGPR spills.

Extraction: ``llvm-objcopy --dump-section .hip_fatbin`` on the library (one offload bundle per translation unit, one
after the other), each bundle split off at its ``__CLANG_OFFLOAD_BUNDLE__`` magic and unbundled for gfx950 with
``clang-offload-bundler``, then ``llvm-readelf --notes`` for the kernel metadata.  Tools from ``$ROCM_PATH/llvm/bin``
(default /opt/rocm).
"""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "motion-policy-networks_amd", "mpinets_amd", "libmpinets_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

# kernels whose correctness depends on a counted vmcnt wait: demangled name prefix -> instantiations that must exist
COUNTED_WAIT_KERNELS = {
    "sa3_front_bf16x3_kernel<": 2,  # <false>, <true> (PROBE)
    "linear_bf16x3_pairs_kernel<0>": 1,
    "linear_bf16x3_pairs_kernel<1>": 1,
    "linear_bf16x3_pairs_kernel<2>": 1,
    "linear_bf16x3_pairs_kernel<3>": 1,
}
NO_SCRATCH_FIELDS = (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def _tool(name):
    path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    assert os.path.exists(path), f"{path} not found (ROCm's LLVM tools read the code objects)"
    return path


def demangle_head(sym):
    """``_Z<len><name>I<template args>E...`` -> ``name<args>`` for integer / bool literal arguments (``Li3E``, ``Lb0E``):
    enough to name the kernels of this library by their demangled prefix without a demangler on the box."""
    m = re.match(r"_Z(\d+)", sym)
    if not m:
        return sym
    n, p = int(m.group(1)), m.end()
    name, rest = sym[p:p + n], sym[p + n:]
    if not rest.startswith("I"):
        return name
    args = re.match(r"I((?:L[ib]n?\d+E)+)E", rest)
    if not args:
        return name + "<?>"
    vals = []
    for kind, neg, v in re.findall(r"L([ib])(n?)(\d+)E", args.group(1)):
        vals.append(("true" if v != "0" else "false") if kind == "b" else ("-" if neg else "") + v)
    return f"{name}<{', '.join(vals)}>"


def code_objects(so_path, tmp):
    """-> paths of the gfx950 code objects of ``so_path`` (one per translation unit), unbundled into directory ``tmp``."""
    paths = []
    fb = os.path.join(tmp, "fatbin")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", so_path, os.path.join(tmp, "so")],
                   check=True, capture_output=True)
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)]
    assert starts and starts[0] == 0, "no offload bundle at the start of .hip_fatbin"
    for i, s in enumerate(starts):
        e = starts[i + 1] if i + 1 < len(starts) else len(data)
        bpath, cpath = os.path.join(tmp, f"b{i}"), os.path.join(tmp, f"b{i}.co")
        with open(bpath, "wb") as f:
            f.write(data[s:e])
        subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--unbundle", f"--targets={TARGET}",
                        f"--input={bpath}", f"--output={cpath}"], check=True, capture_output=True)
        paths.append(cpath)
    return paths


def kernel_metadata(so_path):
    """-> {mangled kernel name: {metadata field: value string}} over every gfx950 code object in ``so_path``."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for cpath in code_objects(so_path, tmp):
            notes = subprocess.run([_tool("llvm-readelf"), "--notes", cpath], check=True, capture_output=True,
                                   text=True).stdout
            # amdhsa.kernels is a YAML list: an entry starts at "  - .<key>", its scalar fields sit at 4 spaces
            for entry in re.split(r"\n  - ", notes.split("amdhsa.kernels:", 1)[-1])[1:]:
                fields = dict(re.findall(r"^ {0,4}(\.[a-z_]+):[ \t]+(\S+)[ \t]*$", "    " + entry, flags=re.M))
                if ".name" in fields:
                    out[fields[".name"]] = fields
    return out


@pytest.fixture(scope="module")
def metadata():
    assert os.path.exists(LIB), f"{LIB} not built (run __graft_entry__.build())"
    md = kernel_metadata(LIB)
    assert len(md) >= 50, f"only {len(md)} kernels found in the gfx950 code objects"
    return md


def test_demangle_head():
    assert demangle_head("_Z26linear_bf16x3_pairs_kernelILi3EEvPKDF16biS1_iiPKfiiiPfiPDF16bi") == \
        "linear_bf16x3_pairs_kernel<3>"
    assert demangle_head("_Z23sa3_front_bf16x3_kernelILb1EEvPKfiPKhPDF16biPx") == "sa3_front_bf16x3_kernel<true>"
    assert demangle_head("_Z17split_bf16_kernelPKfiliiPDF16bi") == "split_bf16_kernel"


def test_metadata_reader_sees_scratch_fields(metadata):
    """Every kernel entry carries the three fields the check below reads (a format change fails here, not silently)."""
    for name, f in metadata.items():
        for key in NO_SCRATCH_FIELDS:
            assert key in f, f"{name}: no {key} in its metadata"


@pytest.mark.parametrize("prefix", sorted(COUNTED_WAIT_KERNELS))
def test_counted_wait_kernels_use_no_scratch(metadata, prefix):
    hits = {demangle_head(n): f for n, f in metadata.items() if demangle_head(n).startswith(prefix)}
    assert len(hits) == COUNTED_WAIT_KERNELS[prefix], \
        f"expected {COUNTED_WAIT_KERNELS[prefix]} instantiation(s) of {prefix}*, found {sorted(hits)}"
    for name, f in hits.items():
        bad = {k: f[k] for k in NO_SCRATCH_FIELDS if int(f[k]) != 0}
        assert not bad, (f"{name} uses scratch {bad}: its counted vmcnt wait would no longer cover its DMA loads "
                         "(spill loads / stores count on the same counter)")
