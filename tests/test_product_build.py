"""The product library ships only the kernels the product paths launch and reads
no environment (the measured alternatives and their OKV_* knobs live in the
ablation build, -DOKV_ABLATE).  Checked on the built files, no GPU needed:
kernel symbol names of the embedded gfx950 code object and the string
literals of the host code are plain bytes in the shared object."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(ROOT, "objectkv_amd", "libokv_sst.so")
ABLATE = os.path.join(ROOT, "objectkv_amd", "libokv_sst_ablate.so")

# kernels of the measured alternative forms: ablation build only
ABLATION_ONLY = [b"okv_value_sweep_kernel", b"okv_rows_kernel", b"okv_gather_staged_kernel",
                 b"okv_gather_kernel", b"okv_tile_kernel_w7", b"okv_scan_kernel",
                 b"okv_tile_kernel_diag",
                 # round 4's measured-and-not-kept forms
                 b"okv_decode_stream_kernel", b"okv_enc_plan_kernel", b"fused_prefix_lookback",
                 # round 6's
                 b"okv_group_kernel", b"okv_tile_kernel_skip",
                 # the encode pack kernels' measured arms
                 b"okv_enc_pack_lds_arm_kernel", b"okv_enc_pack_region_arm_kernel"]
KNOBS = [b"OKV_GATHER_THREADS", b"OKV_GATHER_GRID", b"OKV_DECODE_FUSED", b"OKV_GATHER_STAGED",
         b"OKV_VALUE_SWEEP", b"OKV_TILE", b"OKV_ZSTD_GENERAL", b"OKV_ZSTD_PROF",
         b"OKV_ENC_VARIANT", b"OKV_ENC_IMAGE", b"OKV_DECODE_PIECES", b"OKV_DECODE_STREAM",
         b"OKV_SMALL_PIECE_MB", b"OKV_COUNT_PREFETCH", b"OKV_ENC_ONEPASS", b"OKV_ENC_META_FUSED",
         b"OKV_ZSTD_HUF_BLOCKS", b"OKV_DECODE_GROUP", b"OKV_ZSTD_PRO_GRID", b"OKV_ZSTD_EXEC_GRID"]
# the zstd stage's diagnostic reports (okv_zstd_ablate_host.inc): ablation build only
ZSTD_REPORTS = [b"[zstd prof]", b"[zstd exec]", b"[zstd pro]"]


def _bytes(path):
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not built")
    with open(path, "rb") as f:
        return f.read()


def test_product_ships_one_tile_pass_form():
    data = _bytes(PRODUCT)
    forms = set(re.findall(rb"_ZN3okv15okv_tile_kernelI[A-Za-z0-9_]+", data))
    assert forms == {b"_ZN3okv15okv_tile_kernelILj16384ELj256ELb1EEEvNS_10CopyParamsEjj"}, forms
    for name in ABLATION_ONLY:
        assert name not in data, name
    # the shipping kernels are all there
    for name in (b"okv_count_kernel", b"okv_gather_small_kernel", b"okv_decode_fused_kernel",
                 b"okv_copy_kernel", b"okv_index_kernel", b"okv_hash_kernel",
                 b"okv_enc_pack_lds_kernel", b"okv_zstd_seq_kernel", b"okv_zstd_exec_kernel",
                 b"okv_merge_rank"):
        assert name in data, name


def test_product_source_holds_only_product_kernels():
    """The shipped source is the shipped code: the measured alternatives and
    the tile pass's diagnostic arms live in okv_decode_ablate.inc, which
    okv_decode.hip includes only under -DOKV_ABLATE."""
    src = open(os.path.join(ROOT, "objectkv_amd", "csrc", "okv_decode.hip")).read()
    for name in ("okv_value_sweep_kernel", "okv_rows_kernel", "okv_gather_staged_kernel",
                 "okv_gather_kernel", "tile_pass_diag", "okv_tile_kernel_diag"):
        assert not re.search(r"void\s+" + name + r"\s*\(", src), name
    for arm in ("kProbe", "kDirect", "kChunk", "kDiag == 1", "kDiag == 4", "kDiag == 5"):
        assert arm not in src, arm
    for inc_name in ("okv_decode_ablate.inc", "okv_decode_ablate_host.inc",
                     "okv_decode_ablate_lb.inc"):
        inc = src.index(f'#include "{inc_name}"')
        assert src.rfind("#ifdef OKV_ABLATE", 0, inc) > src.rfind("#endif", 0, inc), inc_name
    # round 4's arms are in the includes, not in the product translation units
    for name in ("okv_decode_stream_kernel", "launch_plan_pieces", "launch_count_piece",
                 "piece_params", "okv_group_kernel", "ensure_group",
                 # the ablation dispatch: its selector, its tile forms, its knobs
                 "ablate_decode", "ablate_open", "ablate_close", "ablate_launch_tile",
                 "ablate_count_prefetch", "launch_tile_t", "tile_form", "okv_debug_probe"):
        assert not re.search(r"\b" + name + r"\s*\([^;]*\)\s*\{", src), name
    enc = open(os.path.join(ROOT, "objectkv_amd", "csrc", "okv_encode.hip")).read()
    for name in ("okv_enc_plan_kernel", "enc_plan_fast"):
        assert not re.search(r"\b" + name + r"\s*\([^;]*\)\s*\{", enc), name
    for inc_name in ("okv_encode_ablate.inc", "okv_encode_ablate_host.inc",
                     "okv_encode_ablate_pack.inc"):
        inc = enc.index(f'#include "{inc_name}"')
        assert enc.rfind("#ifdef OKV_ABLATE", 0, inc) > enc.rfind("#endif", 0, inc), inc_name


def test_decode_ablation_enters_through_hooks():
    """The ablation arms are out of line: okv_decode.hip names OKV_ABLATE for
    the three includes, the two device-side stamp macros and at most five
    single-line host hooks, one of them in decode_device, whose body is the
    product dispatcher and fits two screens."""
    src = open(os.path.join(ROOT, "objectkv_amd", "csrc", "okv_decode.hip")).read()
    assert src.count("#ifdef OKV_ABLATE") <= 10
    body = src[src.index("\nint decode_device("):]
    body = body[:body.index("\n}\n")]
    assert body.count("OKV_ABLATE") <= 1
    assert body.count("\n") <= 120


def test_product_reads_no_environment():
    data = _bytes(PRODUCT)
    for knob in KNOBS + ZSTD_REPORTS:
        assert knob not in data, knob
    dyn = subprocess.run(["nm", "-D", "--undefined-only", PRODUCT], capture_output=True,
                         text=True, check=True).stdout
    assert not re.search(r"\bgetenv\b", dyn), "the product library imports getenv"


def test_ablation_build_carries_the_alternatives():
    data = _bytes(ABLATE)
    for name in (b"okv_value_sweep_kernel", b"okv_gather_staged_kernel", b"okv_tile_kernel_w7",
                 b"okv_decode_stream_kernel", b"okv_enc_plan_kernel",
                 b"okv_enc_pack_lds_arm_kernel", b"okv_enc_pack_region_arm_kernel"):
        assert name in data, name
    for knob in [b"OKV_VALUE_SWEEP", b"OKV_TILE", b"OKV_ZSTD_PROF"] + ZSTD_REPORTS:
        assert knob in data, knob


def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def test_pack_kernels_are_the_product_form_only():
    """The encode pack kernels are what the product launches, nothing else:
    one non-template symbol each in the product library, no variant parameter
    or knob in okv_encode.hip, okv_enc_pack_lds_kernel a short sequence of
    phases; the decode copy helpers carry no variant parameter either."""
    data = _bytes(PRODUCT)
    for name, mangled in ((b"okv_enc_pack_lds_kernel",
                           b"_ZN3okv23okv_enc_pack_lds_kernelENS_10PackParamsEmj"),
                          (b"okv_enc_pack_region_kernel",
                           b"_ZN3okv26okv_enc_pack_region_kernelENS_10PackParamsEmj")):
        forms = set(re.findall(rb"_ZN3okv\d+" + name + rb"[A-Za-z0-9_]*", data))
        assert forms == {mangled}, forms
    csrc = os.path.join(ROOT, "objectkv_amd", "csrc")
    enc = _strip_comments(open(os.path.join(csrc, "okv_encode.hip")).read())
    for word in ("kMeta", "kOverlap", "OKV_ENC_VARIANT", "template <int V"):
        assert not re.search(r"\b" + word + r"\b", enc), word
    dec = _strip_comments(open(os.path.join(csrc, "okv_decode.hip")).read())
    assert "template <int V" not in dec
    m = re.search(r"\n[^\n;{}]*\bokv_enc_pack_lds_kernel\s*\([^)]*\)\s*\{.*?\n\}", enc, flags=re.S)
    assert m and "__global__" in m.group(0)
    assert m.group(0).strip("\n").count("\n") + 1 <= 25


def test_tile_pass_is_a_sequence_of_phases():
    """The product tile pass carries no ablation arm: tile_pass is a short
    sequence of phase calls with no loop of its own, the helpers only the
    measured forms use live in okv_decode_ablate.inc, and those forms call the
    product's phases instead of repeating them (the scalar trip is stated once)."""
    csrc = os.path.join(ROOT, "objectkv_amd", "csrc")
    dec = _strip_comments(open(os.path.join(csrc, "okv_decode.hip")).read())
    for word in ("kSkip", "kSector", "kKeyRound", "kDiag"):
        assert word not in dec, word
    for name in ("boundary_chunk", "sweep_handoff", "sweep_safe", "tile_chunk_pieces"):
        assert not re.search(r"\b" + name + r"\s*\([^;]*\)\s*\{", dec), name
    m = re.search(r"\n[^\n;{}]*\btile_pass\s*\([^)]*\)\s*\{.*?\n\}", dec, flags=re.S)
    assert m and "__device__" in m.group(0)
    assert m.group(0).strip("\n").count("\n") + 1 <= 60
    assert "for (" not in m.group(0) and "while (" not in m.group(0)
    trips = {}
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if os.path.isfile(path):
            n = open(path, errors="replace").read().count('asm volatile("" ::"s"(off)')
            if n:
                trips[name] = n
    assert trips == {"okv_decode.hip": 1}, trips


def test_staged_block_machinery_is_stated_once():
    """A block staged in LDS has one byte source (okv_kernels.hpp's Staged), and one
    speculative header walk, walk_staged_to; okv_point_kernel is a short sequence of
    phases with no loop of its own over records."""
    csrc = os.path.join(ROOT, "objectkv_amd", "csrc")
    ballots = []
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if not os.path.isfile(path):
            continue
        src = open(path, errors="replace").read()
        for word in ("StageWin", "LdsSrc", "StageSrc"):
            assert word not in src, (name, word)
        if name.endswith((".hip", ".hpp")):
            ballots += [(name, m.start()) for m in re.finditer(r"__ballot\(brk\)", src)]
    assert [name for name, _ in ballots] == ["okv_kernels.hpp"], ballots
    hpp = open(os.path.join(csrc, "okv_kernels.hpp")).read()
    start = hpp.rfind("void walk_staged_to(", 0, ballots[0][1])
    assert start >= 0 and "\n}\n" not in hpp[start:ballots[0][1]]  # inside that definition
    dec = open(os.path.join(csrc, "okv_decode.hip")).read()
    m = re.search(r"\n[^\n;{}]*\bokv_point_kernel\s*\([^)]*\)\s*\{.*?\n\}", dec, flags=re.S)
    assert m and "__global__" in m.group(0)
    assert m.group(0).strip("\n").count("\n") + 1 <= 120
    assert "while (" not in m.group(0)


def test_host_mode_staging_is_stated_once():
    """The batched calls' host mode is okv_stage.hpp's: one key check, one 256-byte
    rounding, one KeyRows; the CU count is okv_ctx.hpp's cu_count."""
    csrc = os.path.join(ROOT, "objectkv_amd", "csrc")
    code = {name: _strip_comments(open(os.path.join(csrc, name), errors="replace").read())
            for name in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, name))}
    callers = ("okv_bloom.hip", "okv_get.hip", "okv_snap.hip", "okv_seek.hip")
    assert {n: c.count("lies outside key_arena_bytes") for n, c in code.items()
            if "lies outside key_arena_bytes" in c} == {"okv_stage.hpp": 1}
    assert {n: len(re.findall(r"\bstruct KeyRows\b", c)) for n, c in code.items()
            if re.search(r"\bstruct KeyRows\b", c)} == {"okv_stage.hpp": 1}
    for name in callers:
        assert "+ 255) & ~" not in code[name], name
        assert not re.search(r"\bal(256)?\s*(=|\()", code[name]), name
        assert "hipDeviceAttributeMultiprocessorCount" not in code[name], name
        assert "okv_stage.hpp" in code[name] or "okv_get_kernels.hpp" in code[name], name
    assert code["okv_stage.hpp"].count("+ 255) & ~") == 1
    assert code["okv_ctx.hpp"].count("hipDeviceAttributeMultiprocessorCount") == 1


def test_zstd_stage_owns_its_scratch_and_diagnostics_are_out_of_line():
    """okv_zstd.hip's host part (everything after its last kernel) is the
    product sequence: the knobs, the profiling and the reports live in
    okv_zstd_ablate_host.inc, entered through hooks; the stage's scratch is
    zst::Scratch in okv_zstd.hip, and neither the shared context nor
    okv_decode.hip names a field of it."""
    csrc = os.path.join(ROOT, "objectkv_amd", "csrc")
    src = open(os.path.join(csrc, "okv_zstd.hip")).read()
    inc = src.index('#include "okv_zstd_ablate_host.inc"')
    assert src.rfind("#ifdef OKV_ABLATE", 0, inc) > src.rfind("#endif", 0, inc)
    last_kernel = [m.start() for m in re.finditer(r"__global__", src)][-1]
    assert inc > last_kernel
    host = _strip_comments(src[last_kernel:])
    for word in (r"\bknob\s*\(", r"\bgetenv\b", r"\batoi\b", r"\bfprintf\b", r"\bstatic\b"):
        assert not re.search(word, host), word
    assert src[last_kernel:].count("OKV_ABLATE") <= 3
    m = re.search(r"\nint zstd_run\([^)]*\)\s*\{\n(.*?)\n\}\n", src, flags=re.S)
    assert m and m.group(1).count("\n") + 1 <= 80
    # the sequence launches each kernel from one place, the stream stage through launch_huf
    launched = re.findall(r"hipLaunchKernelGGL\(\s*(\w+)", m.group(1))
    assert len(launched) == len(set(launched)) == 5, launched
    assert len(re.findall(r"hipLaunchKernelGGL\(\s*okv_zstd_huf_kernel\b", host)) == 1
    assert "struct Scratch" in host and "#define" not in host
    ctx = _strip_comments(open(os.path.join(csrc, "okv_ctx.hpp")).read())
    assert not re.findall(r"\bz_[a-z_]+", ctx)
    assert not re.search(r"\bkZstdLitBytes\b|\blaunch_zstd_\w+|\bzstd_run\b", ctx)
    dec = _strip_comments(open(os.path.join(csrc, "okv_decode.hip")).read())
    assert not re.findall(r"\bz_[a-z_]+", dec)


def test_allocation_calls_are_confined():
    """Every device and pinned allocation is an okv::Buf (okv_buf.hpp): outside
    comments, the HIP allocation calls appear in that header and in the four
    public allocators of okv_decode.hip, nowhere else under csrc/."""
    csrc = os.path.join(ROOT, "objectkv_amd", "csrc")
    calls = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")
    public = ("okv_device_alloc", "okv_device_free", "okv_host_alloc", "okv_host_free")
    seen_public = set()
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if name == "okv_buf.hpp" or not os.path.isfile(path):
            continue
        src = _strip_comments(open(path, errors="replace").read())
        if name == "okv_decode.hip":
            for fn in public:  # cut the allocator's definition out: signature to closing brace
                m = re.search(r"\n[^\n;{}]*\b" + fn + r"\s*\([^)]*\)\s*\{.*?\n\}", src, flags=re.S)
                assert m, fn
                assert calls.search(m.group(0)), fn
                seen_public.add(fn)
                src = src[:m.start()] + src[m.end():]
        found = calls.findall(src)
        assert not found, (name, found)
    assert seen_public == set(public)
    assert calls.search(_strip_comments(open(os.path.join(csrc, "okv_buf.hpp")).read()))
