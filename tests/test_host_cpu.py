"""CPU-only checks of the host side: the C-ABI library loads and exports every declared symbol,
model-directory parsing/validation, the weight packer + MFMA slot layout (emulated in numpy against
the oracle), and that the product path refuses to run without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import adanerf_oracle as O
from conftest import BINS_CASES, ENCODING_CASES, ROOT, TOPOLOGY_CASES, case_weights, load_case
from mfma_emulation import (PackedNet, pack_weights, run_sampling_net, run_sampling_net_generic, run_shading_net,
                            run_shading_net_generic)

import adanerf_amd
from adanerf_amd import renderer as R


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    return sorted(set(re.findall(r"\b(adanerf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(lib):
    names = _header_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libadanerf_hip.so does not export %s" % n
    assert set(R.EXPORTS) <= set(names)


def test_dependency_list_is_the_include_closure():
    """adanerf_amd/build.py: what `_stale()` watches and `source_hash()` stamps profiles with is every file the library's
    translation units reach through #include "..." -- derived here a second way (the preprocessor's own dependency output would
    need hipcc's headers; a plain scan of the text is enough for quoted includes).  Round 3 shipped with k_generic16.hip.hpp
    missing from a hand-kept list."""
    from adanerf_amd import build as B
    csrc = B.CSRC
    seen, todo = set(), list(B.LIB_SOURCES)
    while todo:
        rel = os.path.normpath(todo.pop())
        if rel in seen:
            continue
        if os.path.basename(rel).startswith("x_") and not os.path.exists(os.path.join(csrc, rel)):
            assert os.path.exists(os.path.join(ROOT, "tools", "experiments", os.path.basename(rel)))      # experiment-only, reached through -I
            continue
        seen.add(rel)
        for line in open(os.path.join(csrc, rel), errors="replace"):
            m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
            if m:
                todo.append(os.path.join(os.path.dirname(rel), m.group(1)))
    assert sorted(seen) == list(B.LIB_DEPS)
    assert "k_generic16.hip.hpp" in B.LIB_DEPS and os.path.normpath("../../include/adanerf_hip.h") in B.LIB_DEPS
    every_header = {f for f in os.listdir(csrc) if f.endswith((".hpp", ".h"))}
    assert every_header <= set(B.LIB_DEPS), "headers in csrc/ that no translation unit includes: %s" % sorted(every_header - set(B.LIB_DEPS))
    assert not any(f.startswith("x_") for f in os.listdir(csrc)), "experiment-only headers belong in tools/experiments/"
    for src in B.LIB_SOURCES:      # device code stays in the .hip units, all of which the ISA tests below compile
        if src.endswith(".cpp"):
            reached = [d for d in B.include_closure([src]) if d.endswith(".hip.hpp")]
            assert not reached, "%s reaches device headers: %s" % (src, reached)
    h0 = B.source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h0)


def test_no_kernel_goes_through_the_lds_crossbar_for_lane_exchanges():
    """profiles/r03_dense_shard_flake.md: a float wave sum through __shfl_xor (ds_bpermute_b32) lost one lane's term on ~1 ray in 10^4, only next
    to other contexts on the same GPU, and no root cause was found.  The avoidance is complete by construction: every lane exchange
    of the library is DPP / permlane / readlane (k_common.hip.hpp), none is a shuffle.  This test keeps it that way at the source level
    (the experiment-only header x_handsched.hip.hpp is not part of the shipped library) and, when the device assembly of the main
    translation unit is at hand (tools/asm_report.py writes it), at the instruction level."""
    from adanerf_amd import build as B
    pat = re.compile(r"__shfl\w*\s*\(|ds_bpermute|ds_permute|__builtin_amdgcn_ds_bpermute|__builtin_amdgcn_ds_permute")
    hits = []
    for rel in B.LIB_DEPS:
        if os.path.basename(rel).startswith("x_") or rel.endswith(".h"):
            continue
        for n, line in enumerate(open(os.path.join(B.CSRC, rel), errors="replace"), 1):
            code = line.split("//", 1)[0]
            if pat.search(code):
                hits.append("%s:%d: %s" % (rel, n, line.strip()))
    assert not hits, "lane exchanges through the LDS crossbar:\n" + "\n".join(hits)
    asm = "/tmp/adanerf_adanerf_hip.hip.s"
    if os.path.exists(asm) and os.path.getmtime(asm) >= max(os.path.getmtime(os.path.join(B.CSRC, d)) for d in B.LIB_DEPS):
        text = open(asm).read()
        assert "ds_bpermute" not in text and "ds_permute" not in text


def _device_assembly():
    """gfx950 assembly of every .hip translation unit of the library (build.LIB_SOURCES) with the shipped flags, cached in /tmp under the source hash (one ~60 s
    compile per change of the sources); None without hipcc."""
    import shutil
    import subprocess
    from adanerf_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    texts = []
    for src in (s for s in B.LIB_SOURCES if s.endswith(".hip")):
        out = "/tmp/adanerf_isa_%s_%s.s" % (B.source_hash(), src)
        if not os.path.exists(out):
            tmp = out + ".tmp%d" % os.getpid()
            subprocess.run([hipcc] + B.HIPCC_FLAGS + B.TU_FLAGS.get(src, []) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                            os.path.join(B.CSRC, src), "-o", tmp], check=True, stderr=subprocess.DEVNULL)
            os.replace(tmp, out)
        texts.append(open(out).read())
    return "\n".join(texts)


def test_device_code_has_no_crossbar_exchange_and_no_lds_dma_outliving_its_workgroup():
    """Instruction-level companions of the test above, on the shipped flags' gfx950 assembly: (1) no ds_bpermute / ds_permute
    in any kernel; (2) every kernel that copies global -> LDS with buffer_load ... lds (the weight rings and tile stages of the MLP
    kernels) drains its vector-memory counter -- s_waitcnt vmcnt(0) -- after the last such copy in program order and before its final
    s_endpgm: no LDS-DMA write can land after the workgroup's LDS allocation has been handed to another workgroup."""
    text = _device_assembly()
    if text is None:
        pytest.skip("no hipcc")
    assert "ds_bpermute" not in text and "ds_permute" not in text
    kernels = re.split(r"\n\s*\.globl\s+", text)
    checked = []
    for k in kernels:
        name = k.split("\n", 1)[0].strip()
        body = k.split(".end_amdhsa_kernel")[0] if ".amdhsa_kernel" in k else k
        lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
        lines = [ln for ln in lines if ln and not ln.startswith(".")]
        dma = [i for i, ln in enumerate(lines) if re.match(r"(buffer|global)_load_\w+ .*\blds\b", ln)]
        if not dma:
            continue
        ends = [i for i, ln in enumerate(lines) if ln.startswith("s_endpgm")]
        assert ends, name
        tail = lines[dma[-1] + 1:ends[-1]]
        assert any(re.match(r"s_waitcnt\b.*vmcnt\(0\)", ln) for ln in tail), "%s: LDS-DMA in flight at s_endpgm" % name
        checked.append(name)
    # the kernels this is about: both 8 x 256 engines, the fp16 sampling pass, the run-time-shaped 16-bit kernels
    for frag in ("shade_mlp16x2_kernel", "sample_mlp16x3_kernel", "sample_mlp16_kernel", "shade_mlp16_gen_staged_kernel",
                 "sample_mlp16x3_gen_kernel"):
        assert any(frag in n for n in checked), frag


def test_device_code_has_no_packed_fp32_valu():
    """Round 5: the shipped flags' gfx950 assembly holds no v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32.  The round-3
    reproducibility fault needs SLP-packed fp32 code around a packed product (tools/probes/pk_mul_fault/README.md: the failing kernel passes
    when built with -fno-slp-vectorize, with or without a hand-written v_pk_mul_f32 of its own), and beside MFMAs a packed fp32 op costs more
    than the two scalar ones it replaces (MI355X_MICROARCH.md); the library is built with -fno-slp-vectorize and its one explicit float2
    computation (split_pack) is scalar."""
    from adanerf_amd import build as B
    assert "-fno-slp-vectorize" in B.HIPCC_FLAGS
    text = _device_assembly()
    if text is None:
        pytest.skip("no hipcc")
    hits = re.findall(r"v_pk_(?:mul|add|fma)_f32", text)
    assert not hits, "%d packed-fp32 instructions in the device code" % len(hits)
    assert text.count("v_mfma_f32_32x32x16") > 10000      # (the text really is the library's assembly)


def test_every_inline_asm_conversion_is_behind_its_accumulators_guard():
    """hipcc's hazard recogniser inserts no wait states between an MFMA and an INLINE-ASM consumer of its result (it pads compiler-visible VALU
    only): the clamped bf16 conversion of the 16-bit shading kernels (k_mlp16.hip.hpp epilogue_quad_16) therefore names, as an operand, the SGPR a
    v_readfirstlane of the same accumulator wrote (mfma_guard) -- a visible VALU read the recogniser does pad.  On the assembly: every
    `v_cvt_pk_bf16_f32 ... clamp` carries its guard's SGPR in the trailing comment, and walking back from it the instruction that wrote that SGPR
    last is a v_readfirstlane_b32 of a register of the very accumulator tile (16 consecutive VGPRs written by one MFMA) both sources belong to."""
    text = _device_assembly()
    if text is None:
        pytest.skip("no hipcc")
    checked = 0
    for k in re.split(r"\n\s*\.globl\s+", text):
        if "clamp" not in k:
            continue
        lines = k.split("\n")
        for i, ln in enumerate(lines):
            m = re.match(r"\s+v_cvt_pk_bf16_f32 v\d+, v(\d+), v(\d+) clamp", ln)
            if not m:
                continue
            g = re.search(r"guard (s\d+|vcc_lo|vcc_hi)", lines[i + 1]) if i + 1 < len(lines) else None      # the allocator may pick a VCC half
            assert g, "clamped conversion without a guard operand: %s" % ln
            a, b = int(m.group(1)), int(m.group(2))
            for j in range(i - 1, -1, -1):      # the last write of the guard's SGPR
                w = re.match(r"\s+(\S+) %s, v(\d+)" % g.group(1), lines[j])
                if w:
                    assert w.group(1) == "v_readfirstlane_b32", lines[j]
                    src = int(w.group(2))
                    # the MFMA that wrote the guard's source: its 16-register destination must hold both conversion sources
                    for q in range(j - 1, -1, -1):
                        mm = re.match(r"\s+v_mfma_\S+ v\[(\d+):(\d+)\]", lines[q])
                        if mm and int(mm.group(1)) <= src <= int(mm.group(2)):
                            assert int(mm.group(1)) <= a <= int(mm.group(2)) and int(mm.group(1)) <= b <= int(mm.group(2)), (ln, lines[j], lines[q])
                            break
                    else:
                        raise AssertionError("no MFMA writes the guard's source: %s" % lines[j])
                    checked += 1
                    break
            else:
                raise AssertionError("the guard's SGPR is never written in front of %s" % ln)
    assert checked > 1000      # 832 in the 8 x 256 kernel alone


def test_asm_conversions_are_two_wait_states_ahead_of_the_mfma_that_reads_them():
    """The other edge of the inline-asm conversion: `v_cvt_pk_bf16_f32 ... clamp` is a VALU write the hazard recogniser cannot see, and
    its result is the B operand of the next layer's MFMAs -- a VALU write followed by an MFMA read of the register needs 2 wait states on gfx9 matrix
    cores, which hipcc inserts for compiler-visible VALU only.  On the assembly: between every clamped conversion and the first v_mfma that reads its
    destination VGPR there are at least 2 wait states (an instruction counts 1, `s_nop N` counts N + 1)."""
    text = _device_assembly()
    if text is None:
        pytest.skip("no hipcc")
    checked, closest = 0, 10 ** 9
    rng = re.compile(r"v\[(\d+):(\d+)\]")
    for k in re.split(r"\n\s*\.globl\s+", text):
        if "clamp" not in k:
            continue
        lines = [ln for ln in k.split("\n") if re.match(r"\s+[a-z]", ln)]
        for i, ln in enumerate(lines):
            m = re.match(r"\s+v_cvt_pk_bf16_f32 v(\d+), v\d+, v\d+ clamp", ln)
            if not m:
                continue
            d, states = int(m.group(1)), 0
            for nxt in lines[i + 1:i + 400]:
                ops = nxt.split(None, 1)
                args = ops[1] if len(ops) > 1 else ""
                if ops[0].startswith("v_mfma"):
                    srcs = args.split(",", 1)[1] if "," in args else ""      # everything behind the destination
                    if any(int(a) <= d <= int(b) for a, b in rng.findall(srcs)):
                        assert states >= 2, "an MFMA reads v%d %d wait state(s) behind its clamped conversion in %s" % (d, states, lines[0][:80])
                        closest = min(closest, states)
                        checked += 1
                        break
                # any other instruction that overwrites or consumes the register ends the search (a compiler-visible reader is padded by hipcc)
                if re.search(r"\bv%d\b" % d, args) or any(int(a) <= d <= int(b) for a, b in rng.findall(args)):
                    break
                sn = re.match(r"\s+s_nop (\d+)", nxt)
                states += int(sn.group(1)) + 1 if sn else 1
    assert checked > 300, checked
    print("closest clamped conversion -> MFMA read: %d wait states over %d pairs" % (closest, checked))


def test_counted_bias_waits_have_enough_younger_lds_reads():
    """A tile's bias block is requested a tile ahead by hand-issued ds_read_b128 (k_mlp16.hip.hpp lds_bias_issue) and taken behind
    `s_waitcnt lgkmcnt(N)` with N > 0 (lds_bias_take<YOUNGER>): LDS returns in order, so "at most N operations outstanding" proves the block
    has arrived only if at least N LDS reads were issued BEHIND the request.  On the assembly: walking back from every hand-written counted wait
    to the bias request in front of it, at least N ds_read instructions lie in between -- whatever the scheduler did with the re-fills."""
    text = _device_assembly()
    if text is None:
        pytest.skip("no hipcc")
    checked = 0
    for k in re.split(r"\n\s*\.globl\s+", text):
        lines = k.split("\n")
        in_asm = False
        for i, ln in enumerate(lines):
            if "#ASMSTART" in ln:
                in_asm = True
            elif "#ASMEND" in ln:
                in_asm = False
            m = re.match(r"\s+s_waitcnt lgkmcnt\((\d+)\)", ln)
            if not (in_asm and m and int(m.group(1)) > 0):
                continue
            n, younger = int(m.group(1)), 0
            for j in range(i - 1, -1, -1):
                if re.match(r"\s+ds_read_b128 v\[\d+:\d+\], v\d+ offset:48", lines[j]) and "#ASMEND" in lines[j + 1]:
                    break      # the last read of the request (4 x ds_read_b128 at offsets 0 / 16 / 32 / 48 in one asm statement)
                if re.match(r"\s+ds_read", lines[j]):
                    younger += 1
            else:
                raise AssertionError("counted wait without a bias request in front of it: %s" % ln)
            assert younger >= n, "lgkmcnt(%d) with only %d LDS reads behind the bias request (%s)" % (n, younger, lines[0][:80])
            checked += 1
    assert checked > 100      # 7 per tile and layer in the 8 x 256 kernels


def test_abi_handshake(lib):
    """adanerf_abi_version / adanerf_struct_sizes against the ctypes mirrors (load_library refuses a library that disagrees)."""
    sizes = (C.c_int32 * 3)()
    assert lib.adanerf_abi_version() == R.ABI_VERSION
    assert lib.adanerf_struct_sizes(sizes) == 0
    assert list(sizes) == [C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)]
    src = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    assert int(re.search(r"#define ADANERF_ABI_VERSION (\d+)", src).group(1)) == R.ABI_VERSION


def _opts(**kw):
    o = R._Options(width=64, height=48, batch_rays=0, device_id=0, precision=0, num_samples=0, threshold=-1.0,
                   shard_rank=0, shard_world=1, strip_rows=8)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _model_dir(tmp_path, scene=None, weights=None, name="m"):
    scene = scene or O.Scene((0.5, -1.0, 1.25), (0.7, 0.7, 0.2), (0.15, 8.25), 1.125, 8.75, 8, 0.2)
    weights = weights or O.synthetic_weights(3)
    d = str(tmp_path / name)
    O.write_model_dir(d, scene, weights)
    return d, scene, weights


def test_parse_model_and_info(lib, tmp_path):
    d, sc, _ = _model_dir(tmp_path)
    info = R.Info()
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    o = _opts()
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
    assert (info.width, info.height, info.rays_local, info.batch_rays) == (64, 48, 64 * 48, 64 * 48)
    assert (info.n_in0, info.n_in1, info.num_samples, info.dense, info.use_ndc) == (90, 90, 8, 0, 0)
    assert abs(info.threshold - 0.2) < 1e-7
    assert abs(info.focal - O.focal_from_fov(64, sc.fov)) < 1e-3
    assert abs(info.view_cell_radius - sc.radius) < 1e-6
    # batch semantics of Settings::init (src/settings.cpp:38-46)
    o = _opts(batch_rays=1000)
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0 and info.batch_rays == 1000
    o = _opts(batch_rays=10 ** 8)
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0 and info.batch_rays == 64 * 48
    # overrides
    o = _opts(num_samples=4, threshold=0.3)
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
    assert info.num_samples == 4 and abs(info.threshold - 0.3) < 1e-7


def test_normalisation_names_and_guard_options_are_validated(lib, tmp_path):
    """Every rayMarchNormalization the reference knows parses (src/nerf_raymarch_common.py:233-244), a config without the key too; any other
    name fails with EUNSUPPORTED and says which names exist; a malformed centre and bad guard options are EIO / EINVAL."""
    import dataclasses
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    base = O.Scene((0.5, -1.0, 1.25), (0.7, 0.7, 0.2), (0.15, 8.25), 1.125, 8.75, 8, 0.2)
    for i, norm in enumerate(["None", "Centered", "MaxDepth", "MaxDepthCentered", "LogCentered", "InverseDistCentered", "InverseSqrtDistCentered", ""]):
        d, _, _ = _model_dir(tmp_path, dataclasses.replace(base, normalization=norm, normalization_center=(0.1, 0.2, 0.3) if i % 2 else ()), name="n%d" % i)
        assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts()), C.byref(info)) == 0, norm
    d, _, _ = _model_dir(tmp_path, dataclasses.replace(base, normalization="SqrtCentered"), name="bad")
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts()), C.byref(info)) == -4
    assert b"LogCentered" in lib.adanerf_last_error(None)
    with open(os.path.join(d, "config.ini"), "a") as f:
        f.write("rayMarchNormalization = [InverseSqrtDistCentered, None]\nrayMarchNormalizationCenter = [1.0, 2.0]\n")
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts()), C.byref(info)) == -2
    d, _, _ = _model_dir(tmp_path, base, name="ok")
    for kw in (dict(guard_audit_period=3), dict(guard_audit_period=64), dict(guard_eps=2.0), dict(guard_eps_pair=3.0)):
        assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts(**kw)), C.byref(info)) == -1, kw
    for kw in (dict(guard_audit_period=-1), dict(guard_audit_period=32), dict(guard_eps=0.01, guard_eps_pair=0.015)):
        assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts(**kw)), C.byref(info)) == 0, kw


def test_strip_sharding_partitions_rows(lib, tmp_path):
    d, _, _ = _model_dir(tmp_path)
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    for (w, h, world, strip) in [(800, 800, 8, 8), (1920, 1080, 8, 8), (100, 37, 3, 4), (64, 5, 4, 8)]:
        tot = 0
        mx = 0
        for rank in range(world):
            info = R.Info()
            o = _opts(width=w, height=h, shard_rank=rank, shard_world=world, strip_rows=strip)
            assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
            tot += info.rays_local
            mx = max(mx, info.rays_local)
            assert info.rays_local_max >= info.rays_local
            rmax = info.rays_local_max
        assert tot == w * h
        assert rmax == mx


def test_error_codes_and_messages(lib, tmp_path):
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    o = _opts()
    assert lib.adanerf_host_parse_model(str(tmp_path / "nope").encode(), C.byref(o), C.byref(info)) == -2
    assert b"couldn't open" in lib.adanerf_last_error(None)
    d, _, _ = _model_dir(tmp_path)
    # threshold < 0 unsupported, dense needs N == 128
    cfg = open(os.path.join(d, "config.ini")).read()
    open(os.path.join(d, "config.ini"), "w").write(cfg.replace("adaptiveSamplingThreshold = 0.2", "adaptiveSamplingThreshold = -1.0"))
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == -4
    o2 = _opts(threshold=0.0)
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o2), C.byref(info)) == -4
    o3 = _opts(threshold=0.0, num_samples=128)
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o3), C.byref(info)) == 0 and info.dense == 1
    # raySampleInput: A extra points in the oracle input (accepted: n_in0 grows by A * 63), nonsense values rejected
    open(os.path.join(d, "config.ini"), "w").write(cfg.replace("raySampleInput = [0, 0]", "raySampleInput = [128, 0]"))
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0 and info.n_in0 == 90 + 128 * 63
    open(os.path.join(d, "config.ini"), "w").write(cfg.replace("raySampleInput = [0, 0]", "raySampleInput = [-3, 0]"))
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == -4
    # any F_pos-F_dir up to 16 bands parses (the network input widths follow); beyond that: unsupported
    open(os.path.join(d, "config.ini"), "w").write(cfg.replace("posEncArgs = [10-4, 10-4]", "posEncArgs = [6-3, 12-2]"))
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
    assert (info.n_in0, info.n_in1) == (3 + 36 + 3 + 18, 3 + 72 + 3 + 12)
    open(os.path.join(d, "config.ini"), "w").write(cfg.replace("posEncArgs = [10-4, 10-4]", "posEncArgs = [17-3, 10-4]"))
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == -4
    assert lib.adanerf_host_parse_model(None, C.byref(o), C.byref(info)) == -1


def test_reference_sample_config_forms_parse(lib, tmp_path):
    """Both shipped config.ini forms (the 71-line training config with section headers and the trimmed
    19-key one) parse to the same Config; here a training-style file is synthesised."""
    d, sc, _ = _model_dir(tmp_path)
    cfg = open(os.path.join(d, "config.ini")).read()
    extra = "[Features]\nlayers = [8, 8]\nlayerWidth = [256, 256]\nskips = [, auto]\ndevice = 0\nlosses = [NeRFWeightMultiplicationLoss, MSE]\n"
    open(os.path.join(d, "config.ini"), "w").write("config = /some/path//fine_training.ini\n" + extra +
                                                   cfg.replace("outFeatures = [Raw, RGBARayMarch]", "outFeatures = [RawSigmoid, RGBARayMarch]"))
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    o = _opts()
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
    assert info.num_samples == sc.num_samples


def test_depth_table_matches_oracle(lib, tmp_path):
    lib.adanerf_host_depth_table.argtypes = [C.c_char_p, C.POINTER(R._Options), C.c_void_p]
    for sc in [O.Scene((0, 0, 0), (1, 1, 1), (0.1542, 8.3582), 1.1, 8.8, 8, 0.2),
               O.Scene((0, 0, 0), (1, 1, 1), (-0.4277, 7.0724), 1.5, 8.7, 128, 0.0),
               O.Scene((0, 0, 0), (1, 1, 1), (0.9, 12.0), 1.0, 12.0, 8, 0.2, use_ndc=True, depth_transform="linear",
                       pos_enc=((2, 2), (10, 4)), normalization="None")]:
        w = O.synthetic_weights(1, n_in0=sc.n_in0)
        d, _, _ = _model_dir(tmp_path, sc, w, name="z%d%d" % (sc.num_samples, int(sc.use_ndc)))
        z = np.zeros(128, dtype=np.float32)
        o = _opts()
        assert lib.adanerf_host_depth_table(d.encode(), C.byref(o), z.ctypes.data) == 0, lib.adanerf_last_error(None)
        t = O.dense_t(sc) if sc.threshold == 0.0 else O.bin_t(np.arange(128))
        np.testing.assert_allclose(z, O.to_world_depth(t, sc), rtol=3e-7, atol=1e-6)


@pytest.mark.parametrize("name", BINS_CASES)
def test_fewer_depth_cells_pack_as_absent_bins(lib, tmp_path, name):
    """multiDepthFeatures = D < 128 (reference-generated fixtures): the sampling network packs into 128-wide output rows whose bins D..127 are
    "absent" (zero weights, bias -1e30: no threshold, arg-max or softmax ever picks them); replayed through the kernels' dataflow in numpy
    the first D outputs are the reference's, the selection from the padded rows is the reference's selection, and the depth table has
    cell_size = 1 / D (src/nerf_raymarch_common.py:726-741).  Dense mode, the inverse-CDF sampler and mismatching config / network are refused."""
    import dataclasses
    z, meta, sc = load_case(name)
    wts = case_weights(meta)
    D = sc.depth_bins
    assert D < 128 and z["oracle_out"].shape[1] == D
    d, _, _ = _model_dir(tmp_path, sc, wts, name=name)
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts(width=meta["w"], height=meta["h"])), C.byref(info)) == 0, lib.adanerf_last_error(None)
    n = 64
    nds = z["nds"][:n]
    u = (nds / np.sqrt(np.sum(nds * nds, -1, keepdims=True))).astype(np.float32)
    generic = "layers" in meta.get("syn", {})      # the combined case: odd widths and two skips too -> the run-time-shaped kernels' dataflow
    for prec, tol in ((2, 1e-4), (3, 1e-4)):
        w, b, lay = pack_weights(lib, d, 0, prec)
        if generic:
            orc = run_sampling_net_generic(PackedNet(w, b, lay, prec), u, z["p"][:n], nds, *sc.pos_enc[0])
        else:
            orc = run_sampling_net(PackedNet(w, b, lay, prec), u, z["p"][:n], *sc.pos_enc[0])
        np.testing.assert_allclose(orc[:, :D], z["oracle_out"][:n], rtol=0, atol=tol)
        assert (orc[:, D:] == np.float32(-1e30)).all()
        cnt, bins, wv = O.select_adaptive(orc, sc.num_samples, sc.threshold)
        assert np.array_equal(cnt, z["sel_count"][:n]) and np.array_equal(bins, z["sel_bins"][:n])
    lib.adanerf_host_depth_table.argtypes = [C.c_char_p, C.POINTER(R._Options), C.c_void_p]
    zt = np.zeros(128, dtype=np.float32)
    assert lib.adanerf_host_depth_table(d.encode(), C.byref(_opts()), zt.ctypes.data) == 0
    np.testing.assert_allclose(zt[:D], O.to_world_depth(O.bin_t(np.arange(D), D), sc), rtol=3e-7, atol=1e-6)
    for k, sc_bad in enumerate((dataclasses.replace(sc, threshold=0.0, num_samples=128), dataclasses.replace(sc, sampler="FromClassifiedDepth", losses0="BCEWithLogitsLoss"))):
        dd, _, _ = _model_dir(tmp_path, sc_bad, wts, name="%s_bad%d" % (name, k))
        assert lib.adanerf_host_parse_model(dd.encode(), C.byref(_opts()), C.byref(info)) == -4 and b"multiDepthFeatures" in lib.adanerf_last_error(None)


@pytest.mark.parametrize("precision,tol", [(2, 2e-4), (1, 3e-2), (0, 2e-1)])
def test_packed_shading_net_reproduces_oracle(lib, tmp_path, precision, tol):
    z, meta, sc = load_case("classroom_n8_thr02")
    wts = case_weights(meta)
    d, _, _ = _model_dir(tmp_path, sc, wts)
    w, b, lay = pack_weights(lib, d, 1, precision)
    # bf16: one more record, the output exponents of the scaled packing (pack.cpp scale_layer; the kernels' ReLU is a clamped conversion)
    assert lay.shape[0] == 11 + (1 if precision == 0 else 0)
    if precision == 0:
        assert int(lay[11][3]) == -1 and 0 < int(lay[11][0]) < 100 and 0 < int(lay[11][1]) < 100
    lay_l = lay[:11]
    assert [int(v) for v in lay_l[:, 3]] == [8] * 8 + [9, 4, 1]
    G = 4 if precision == 2 else 8
    assert sum(int(l[2]) // G * int(l[3]) for l in lay_l) * 1024 == w.size
    if precision != 2:
        assert w.size == 1184 * 1024          # kShadeFrags16 in k_mlp16.hip.hpp
        assert b.size == 2496                 # kShadeBiasFloats
    # a few real samples: positions/dirs from the golden case
    count = z["sel_count"].astype(np.int32)
    off, sray, sbin, sw = O.compact(count, z["sel_bins"], z["sel_weight"])
    n = 48
    zw = O.to_world_depth(O.bin_t(sbin[:n].astype(np.int64)), sc)
    feat = O.shading_inputs(z["p"], z["nds"], sray[:n], zw, sc)
    ref = O.shading_mlp(feat, wts.net1)
    x = feat[:, 0:3]
    dpe = feat[:, 63:66]
    net = PackedNet(w, b, lay, precision)
    out = run_shading_net(net, x, dpe)
    np.testing.assert_allclose(out, ref, rtol=0, atol=tol)
    if precision == 0:
        # the scaled packing is exact: the same blob with the scaling undone in float64 arithmetic is out of reach here, but the replay's
        # ReLU outputs stayed <= 1 (asserted layer by layer) with head-room to spare -- the row-sum bound is loose by construction
        assert net.scaled and 0.0 < net.max_relu_out <= 0.5


def test_packed_sampling_net_reproduces_oracle(lib, tmp_path):
    for name in ["classroom_n8_thr02", "ndc_synthetic_n8"]:
        z, meta, sc = load_case(name)
        wts = case_weights(meta)
        d, _, _ = _model_dir(tmp_path, sc, wts, name=name)
        fp, fd = sc.pos_enc[0]
        n = 64
        nds = z["nds"][:n]
        u = (nds / np.sqrt(np.sum(nds * nds, -1, keepdims=True))).astype(np.float32)
        # exact fp32 fragments, the fp16 hi/lo' split pairs, and the plain fp16 fragments of the opt-in speed mode
        for precision, atol in ((2, 5e-5), (3, 5e-5), (1, 1e-2)):
            w, b, lay = pack_weights(lib, d, 0, precision)
            assert w.size == sum(int(l[2]) // (4 if precision == 2 else 8) * int(l[3]) for l in lay) * 1024 * (2 if precision == 3 else 1)
            if precision == 1 and fp == 10:
                assert w.size == 880 * 1024          # sample16_frags<10, 4>() in k_sampling16.hip.hpp
            orc = run_sampling_net(PackedNet(w, b, lay, precision), u, z["p"][:n], fp, fd)
            np.testing.assert_allclose(orc, z["oracle_out"][:n], rtol=0, atol=atol)


@pytest.mark.parametrize("name", TOPOLOGY_CASES)
def test_generic_topologies_pack_and_reproduce_the_reference(lib, tmp_path, name):
    """networks the reference's model classes built in other shapes (6 x 128 skip 2; 2 x 128 with 3 x 256
    skip 1; 4 x 128 with raySampleInput = 128) load, pack into fp32 MFMA fragments (topology read off the initializers)
    and -- replayed through the kernels' dataflow in numpy -- reproduce the reference's own sampling-network outputs
    and the oracle's shading outputs; the shading net also in the 16-bit packings."""
    z, meta, sc = load_case(name)
    wts = case_weights(meta)
    d, _, _ = _model_dir(tmp_path, sc, wts, name=name)
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    o = _opts(width=meta["w"], height=meta["h"])
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0 and info.n_in0 == sc.n_in0
    syn = meta["syn"]
    fp, fd = sc.pos_enc[0]
    n = 48
    nds = z["nds"][:n]
    u = (nds / np.sqrt(np.sum(nds * nds, -1, keepdims=True))).astype(np.float32)
    w, b, lay = pack_weights(lib, d, 0, 2)
    assert lay.shape[0] == syn["layers"][0] + (1 if sc.ray_sample_input else 0)
    pad = lambda w_: 64 if w_ <= 64 else (128 if w_ <= 128 else 256)      # widths without a kernel instantiation run zero-padded (pack.cpp pad_width)
    pw0, pw1 = pad(syn["widths"][0]), pad(syn["widths"][1])
    assert [int(v) for v in lay[:syn["layers"][0], 3]] == [pw0 // 32] * (syn["layers"][0] - 1) + [4]
    rsi_z = O.ray_sample_depths(sc) if sc.ray_sample_input else None
    orc = run_sampling_net_generic(PackedNet(w, b, lay, 2), u, z["p"][:n], nds, fp, fd, rsi_z, sc.depth_range[1])
    np.testing.assert_allclose(orc, z["oracle_out"][:n], rtol=0, atol=1e-4)
    # shading net on a few of the fixture's samples
    count = z["sel_count"].astype(np.int32)
    off, sray, sbin, sw = O.compact(count, z["sel_bins"], z["sel_weight"])
    feat = O.shading_inputs(z["p"], z["nds"], sray[:n], O.to_world_depth(O.bin_t(sbin[:n].astype(np.int64)), sc), sc)
    ref = O.shading_mlp(feat, wts.net1)
    w1, b1, lay1 = pack_weights(lib, d, 1, 2)
    depth, skips = O.shading_topology(wts.net1, 63)
    out = run_shading_net_generic(PackedNet(w1, b1, lay1, 2), feat[:, 0:3], feat[:, 63:66], depth, pw1, skips)
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-4)
    # the shading net packs for the 16-bit engines in every topology (k_generic16.hip.hpp); replayed in bf16 / fp16 it stays
    # within the operand rounding of the oracle
    for prec, tol in ((0, 0.25), (1, 0.03)):
        wq, bq, layq = pack_weights(lib, d, 1, prec)
        outq = run_shading_net_generic(PackedNet(wq, bq, layq, prec), feat[:, 0:3], feat[:, 63:66], depth, pw1, skips)
        assert np.abs(outq - ref).max() < tol and np.sqrt(np.mean((outq - ref) ** 2)) < tol / 6
    # the sampling net: plain 16-bit fragments only for 8 x 256 (ring-streamed kernel); the split-precision pairs for every
    # topology without raySampleInput (sample_mlp16x3_gen_kernel), reproducing the reference's outputs like the fp32 packing
    f = lib.adanerf_host_pack_weights
    wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    default0 = (syn["layers"][0], syn["widths"][0]) == (8, 256) and not sc.ray_sample_input
    rc = f(d.encode(), 0, 1, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
    assert (rc == 0) == default0, rc
    if not default0:
        assert b"16-bit" in lib.adanerf_last_error(None)
    rc = f(d.encode(), 0, 3, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
    assert (rc == 0) == (default0 or not sc.ray_sample_input), rc
    if rc == 0:
        ws, bs, lays = pack_weights(lib, d, 0, 3)
        orc_s = run_sampling_net_generic(PackedNet(ws, bs, lays, 3), u, z["p"][:n], nds, fp, fd)
        np.testing.assert_allclose(orc_s, z["oracle_out"][:n], rtol=0, atol=1e-4)
        np.testing.assert_allclose(orc_s, orc, rtol=0, atol=2e-5)        # 22-bit operands vs the fp32 fragments


@pytest.mark.parametrize("name", ENCODING_CASES)
def test_other_encodings_pack_into_the_catch_all_layout(lib, tmp_path, name):
    """SURVEY 8f N4, encodings: posEncArgs other than 10-4 / 2-2 (here 6-3 / 12-2 and the extremes 16-1 / 1-16, fixtures
    generated by the reference).  Such networks are packed into the 16-band slot layout of the run-time-shaped kernels --
    the bands the model does not have get zero weights (layout.hpp pe_col) -- and, replayed through the kernels' dataflow
    in numpy with all 16 bands evaluated as the device does, reproduce the reference's sampling-network outputs and the
    oracle's shading outputs (the shading net also in bf16 / fp16)."""
    z, meta, sc = load_case(name)
    wts = case_weights(meta)
    d, _, _ = _model_dir(tmp_path, sc, wts, name=name.replace("-", "_"))
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    o = _opts(width=meta["w"], height=meta["h"])
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
    (fp0, fd0), (fp1, fd1) = sc.pos_enc
    assert (info.n_in0, info.n_in1) == (6 + 6 * (fp0 + fd0), 6 + 6 * (fp1 + fd1))
    n = 48
    nds = z["nds"][:n]
    u = (nds / np.sqrt(np.sum(nds * nds, -1, keepdims=True))).astype(np.float32)
    w, b, lay = pack_weights(lib, d, 0, 2)
    assert int(lay[0, 2]) == 2 * 56                        # layer 0: [dir PE | pos PE] in the 16-band layout (56 slots each)
    orc = run_sampling_net_generic(PackedNet(w, b, lay, 2), u, z["p"][:n], nds, 16, 16)
    np.testing.assert_allclose(orc, z["oracle_out"][:n], rtol=0, atol=2e-4)
    count = z["sel_count"].astype(np.int32)
    off, sray, sbin, sw = O.compact(count, z["sel_bins"], z["sel_weight"])
    feat = O.shading_inputs(z["p"], z["nds"], sray[:n], O.to_world_depth(O.bin_t(sbin[:n].astype(np.int64)), sc), sc)
    np.testing.assert_allclose(feat, z["shade_in"][:n], rtol=0, atol=2e-3 * 2 ** max(fp1 - 10, 0))   # the oracle's features are the reference's
    ref = O.shading_mlp(feat, wts.net1, n_pos=3 + 6 * fp1)
    w1, b1, lay1 = pack_weights(lib, d, 1, 2)
    out = run_shading_net_generic(PackedNet(w1, b1, lay1, 2), feat[:, 0:3], feat[:, 3 + 6 * fp1:6 + 6 * fp1], 8, 256, 4, fp=16, fd=16)
    np.testing.assert_allclose(out, ref, rtol=0, atol=3e-4)
    for prec, tol in ((0, 0.25), (1, 0.03)):      # the shading net in the catch-all layout on the 16-bit engine
        wq, bq, layq = pack_weights(lib, d, 1, prec)
        outq = run_shading_net_generic(PackedNet(wq, bq, layq, prec), feat[:, 0:3], feat[:, 3 + 6 * fp1:6 + 6 * fp1], 8, 256, 4, fp=16, fd=16)
        assert np.abs(outq - ref).max() < tol and np.sqrt(np.mean((outq - ref) ** 2)) < tol / 6
    f = lib.adanerf_host_pack_weights
    wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    assert f(d.encode(), 0, 1, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl)) != 0      # plain fp16 sampling: 10-4 / 2-2 only
    assert b"16-bit" in lib.adanerf_last_error(None)
    ws, bs, lays = pack_weights(lib, d, 0, 3)              # the split-precision pairs in the 16-band layout (sample_mlp16x3_gen_kernel)
    assert int(lays[0, 2]) == 2 * 56
    orc_s = run_sampling_net_generic(PackedNet(ws, bs, lays, 3), u, z["p"][:n], nds, 16, 16)
    np.testing.assert_allclose(orc_s, z["oracle_out"][:n], rtol=0, atol=2e-4)
    np.testing.assert_allclose(orc_s, orc, rtol=0, atol=3e-5)


def test_product_path_fails_loudly_without_gpu(lib, tmp_path):
    """No CPU fallback: on a box without a HIP device create() must fail with EDEVICE (on the GPU box
    this test is a no-op)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    d, _, _ = _model_dir(tmp_path)
    r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 64, 48))
    with pytest.raises(adanerf_amd.AdaNeRFError) as ei:
        r.init()
    assert "no HIP device" in str(ei.value) or "hip" in str(ei.value).lower()


def test_settings_batch_semantics():
    S = adanerf_amd.Settings
    assert S("x", 800, 800).resolved_batch() == 640000
    assert S("x", 800, 800, batch_size=80000).resolved_batch() == 80000
    assert S("x", 800, 800, batch_size=10 ** 9).resolved_batch() == 640000
    assert S("x", 800, 800, number_of_batches=8).resolved_batch() == 80000
    assert S("x", 10, 10, number_of_batches=3).resolved_batch() == 34


def test_package_model_dir_writer_round_trips(lib, tmp_path):
    """adanerf_amd.modeldir (the product-side writer bench.py uses) produces files the library's host parser,
    its packer and the oracle's independent reader all agree on."""
    from adanerf_amd import modeldir as M
    n0, n1 = M.random_init_weights(3)
    d = str(tmp_path / "pm")
    scene = dict(view_cell_center=(0.5, -1.0, 1.25), view_cell_size=(0.7, 0.7, 0.2), depth_range=(0.15, 8.25), fov=1.125,
                 max_depth=8.75, num_samples=8, threshold=0.2)
    M.write_model_dir(d, scene, n0, n1)
    sc = O.load_scene(d)
    w = O.load_weights(d)
    assert sc.num_samples == 8 and abs(sc.threshold - 0.2) < 1e-9 and sc.view_cell_center == (0.5, -1.0, 1.25)
    assert all(np.array_equal(v, w.net0[k]) for k, v in n0.items()) and all(np.array_equal(v, w.net1[k]) for k, v in n1.items())
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    o = _opts()
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info)) == 0
    assert info.num_samples == 8 and info.n_in0 == 90
    wq, b, lay = pack_weights(lib, d, 1, 0)
    assert wq.size == 1184 * 1024
    assert np.allclose(M.camera_rotation(100.0, 0.0), O.camera_rotation(100.0, 0.0))
    assert np.allclose(M.camera_rotation(-80.0, 10.0) @ M.camera_rotation(-80.0, 10.0).T, np.eye(3), atol=1e-6)


def test_png_codec_round_trip_and_filters(tmp_path):
    import struct
    import zlib
    from adanerf_amd.png import read_png, write_png
    rng = np.random.default_rng(0)
    for c in (3, 4):
        img = rng.integers(0, 256, size=(17, 23, c), dtype=np.uint8)
        p = str(tmp_path / ("a%d.png" % c))
        write_png(p, img)
        assert np.array_equal(read_png(p), img)
    # hand-build a PNG that uses every scanline filter (what real encoders emit)
    img = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    bpp, stride = 3, 21
    rows = bytearray()
    prev = np.zeros(stride, dtype=np.int32)
    for y in range(5):
        cur = img[y].reshape(-1).astype(np.int32)
        ft = y % 5
        enc = np.zeros(stride, dtype=np.int32)
        for x in range(stride):
            a = cur[x - bpp] if x >= bpp else 0
            b = prev[x]
            cc = prev[x - bpp] if x >= bpp else 0
            if ft == 0:
                pr = 0
            elif ft == 1:
                pr = a
            elif ft == 2:
                pr = b
            elif ft == 3:
                pr = (a + b) >> 1
            else:
                pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                pr = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
            enc[x] = (cur[x] - pr) & 255
        rows += bytes([ft]) + bytes(enc.astype(np.uint8))
        prev = cur

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    p = str(tmp_path / "filters.png")
    comp = zlib.compress(bytes(rows))
    with open(p, "wb") as f:     # two IDAT chunks, like streaming encoders
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 5, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", comp[:10]) + chunk(b"IDAT", comp[10:]) + chunk(b"IEND", b""))
    assert np.array_equal(read_png(p), img)


def test_evaluator_dataset_loader(tmp_path):
    import json
    from adanerf_amd.evaluate import load_dataset, psnr_from_mse
    d = tmp_path / "ds"
    (d / "test").mkdir(parents=True)
    json.dump(dict(resolution=[64, 48], camera_angle_x=1.1, view_cell_center=[0, 0, 0], view_cell_size=[1, 1, 1]),
              open(d / "dataset_info.json", "w"))
    m = np.eye(4)
    m[:3, 3] = [1, 2, 3]
    json.dump(dict(frames=[dict(file_path="./test/00000", transform_matrix=m.tolist())]), open(d / "transforms_test.json", "w"))
    meta, frames = load_dataset(str(d), "test")
    assert (meta["w"], meta["h"]) == (64, 48) and abs(meta["fov"] - 1.1) < 1e-9
    assert np.allclose(frames[0]["pose"], [1, 2, 3]) and np.allclose(frames[0]["rot"], np.eye(3))
    assert frames[0]["image"].endswith(os.path.join("test", "00000.png"))
    assert abs(psnr_from_mse(0.01) - 20.0) < 1e-9


def test_dataset_reader_matches_the_reference_readers(lib, tmp_path):
    """SURVEY 8f N1 pinned: tests/golden/dataset_reader.npz holds a tiny dataset directory (file by file) together with what
    the reference's DatasetInfo / FullyLoadedViewCellDataset (src/datasets.py:146-213, 263-287, 361-365, 479-542) derived
    from it (oracle/gen_golden.py: gen_dataset_reader).  The evaluator's reader and PNG decoder must derive the same:
    resolution, field of view, poses, rotations, image paths and the [0, 1] float colour images bit for bit; the focal
    length is the library's (adanerf_info.focal for that field of view and width)."""
    from conftest import GOLD
    from adanerf_amd.evaluate import load_dataset
    from adanerf_amd.png import read_png
    z = np.load(os.path.join(GOLD, "dataset_reader.npz"))
    d = tmp_path / "ds"
    for k in z.files:
        if k.startswith("file:"):
            f = d / k[5:]
            f.parent.mkdir(parents=True, exist_ok=True)
            f.write_bytes(z[k].tobytes())
    meta, frames = load_dataset(str(d), "test")
    assert (meta["w"], meta["h"]) == (int(z["w"]), int(z["h"])) and meta["fov"] == float(z["fov"])
    names = bytes(z["image_names"]).decode().split("\n")
    assert len(frames) == len(names) == z["poses"].shape[0]
    for i, fr in enumerate(frames):
        assert os.path.relpath(fr["image"], str(d)) == names[i]
        assert fr["pose"].dtype == np.float32 and np.array_equal(fr["pose"], z["poses"][i])
        assert np.array_equal(fr["rot"], z["rotations"][i])
        img = read_png(fr["image"])
        mine = img[:, :, :3].astype(np.float32) / np.float32(255.0)          # what evaluate() compares against (datasets.py:286-287)
        assert np.array_equal(mine, z["color_images"][i])
    # focal length of that camera as the library derives it (src/datasets.py:182)
    sc = O.Scene(view_cell_center=tuple(z["view_cell_center"]), view_cell_size=tuple(z["view_cell_size"]),
                 depth_range=tuple(z["depth_range"]), fov=float(z["fov"]), max_depth=float(z["depth_max"]), num_samples=8, threshold=0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0))
    info = R.Info()
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    o = _opts(width=int(z["w"]), height=int(z["h"]))
    assert lib.adanerf_host_parse_model(md.encode(), C.byref(o), C.byref(info)) == 0
    assert info.focal == np.float32(z["focal"]) and abs(info.fov - float(z["fov"])) < 1e-7


def test_header_is_plain_c_and_links_from_c(lib, tmp_path):
    """include/adanerf_hip.h compiled as C99 with gcc; the program drives the library through the C ABI only and the
    struct sizes match the ctypes mirrors in adanerf_amd/renderer.py."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("gcc not available")
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "c_abi_check")
    src = os.path.join(ROOT, "tests", "c_abi_check.c")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", src, "-L", LIBDIR, "-ladanerf_hip",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    d, _, _ = _model_dir(tmp_path)
    out = subprocess.run([exe, d], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "couldn't open" in out.stdout and "rays=3072" in out.stdout
    sizes = out.stdout.strip().splitlines()[-1]
    assert sizes == "sizeof options=%d info=%d stats=%d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats))


def test_map_entry_points_are_declared_and_exported(lib, tmp_path):
    """adanerf_composite_aux, adanerf_composite_classic_aux, adanerf_disp_map: tests/aux_abi_check.c compiled as C99 against the header,
    linked with the library; a NULL context is refused and nothing is written; no struct changed; the Python host has the wrappers."""
    import inspect
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "aux_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "aux_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "aux(NULL) rc=-1 -1 -1 maps=-7 -7 -7 abi=4"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats))
    for name in ("adanerf_composite_aux", "adanerf_composite_classic_aux", "adanerf_disp_map"):
        assert name in R.EXPORTS and hasattr(lib, name)
    par = lambda f: list(inspect.signature(f).parameters)[1:]
    assert par(R.NeuralRenderer.composite_aux) == ["raw", "sample_w", "ray_offsets", "ray_counts", "sample_key", "n_rays", "rgb_out", "rgba8_out", "depth_out", "acc_out"]
    assert par(R.NeuralRenderer.composite_classic_aux) == ["raw", "sample_z", "rays", "n_rays", "n", "rgb_out", "rgba8_out", "depth_out", "acc_out"]
    assert par(R.NeuralRenderer.disp_map) == ["depth", "acc", "n", "disp_out"]
    assert par(R.NeuralRenderer.composite) == ["raw", "sample_w", "ray_offsets", "ray_counts", "n_rays", "rgb_out", "rgba8_out"]
    assert par(R.NeuralRenderer.composite_classic) == ["raw", "sample_z", "rays", "n_rays", "n", "rgb_out", "rgba8_out"]


def test_balanced_strip_rows():
    from adanerf_amd import sharding as S
    assert S.balanced_strip_rows(800, 1) == 8 and S.balanced_strip_rows(800, 2) == 8 and S.balanced_strip_rows(800, 4) == 8
    assert S.balanced_strip_rows(800, 8) == 5 and S.balanced_strip_rows(1080, 8) == 5
    assert S.balanced_strip_rows(7, 4) == 8          # no balanced height: documented fallback
    for h, world in ((800, 8), (1080, 8), (400, 4)):
        sr = S.balanced_strip_rows(h, world)
        per = [S.rays_local(64, h, sr, world, k) for k in range(world)]
        assert len(set(per)) == 1 and sum(per) == 64 * h


def test_y4m_video_writer(tmp_path):
    from adanerf_amd.evaluate import Y4mWriter
    w, h = 6, 4
    path = str(tmp_path / "v.y4m")
    v = Y4mWriter(path, w, h, fps=25)
    grey = np.full((h, w, 3), 100, np.uint8)
    red = np.zeros((h, w, 3), np.uint8); red[..., 0] = 255
    v.add(grey); v.add(red); v.close()
    data = open(path, "rb").read()
    head, rest = data.split(b"\n", 1)
    assert head.startswith(b"YUV4MPEG2 W6 H4 F25:1") and b"C444" in head
    frame = 6 + 3 * w * h
    assert len(rest) == 2 * frame and rest[:6] == b"FRAME\n" and rest[frame:frame + 6] == b"FRAME\n"
    y0 = np.frombuffer(rest[6:6 + w * h], np.uint8); u0 = np.frombuffer(rest[6 + w * h:6 + 2 * w * h], np.uint8)
    assert (y0 == 100).all() and (u0 == 128).all()                       # grey: Y = value, chroma neutral
    y1 = np.frombuffer(rest[frame + 6:frame + 6 + w * h], np.uint8)
    assert (y1 == 76).all()                                              # BT.601: 0.299 * 255


def test_corrupt_model_files_never_crash(tmp_path):
    """The ONNX-initializer reader and the key=value parser are hand-rolled (format.cpp): truncated, bit-flipped and
    garbage files must come back as an error code (or parse), never as a crash or a hang.  Runs in a child process so
    that a segfault fails the test instead of the test run."""
    import subprocess
    import sys
    from conftest import case_weights, load_case
    z, meta, sc = load_case("classroom_n8_thr02")
    d, _, _ = _model_dir(tmp_path, sc, case_weights(meta))
    script = r"""
import ctypes as C, os, shutil, sys, numpy as np
sys.path.insert(0, sys.argv[1])
from adanerf_amd import renderer as R
lib = R.load_library()
src, work = sys.argv[2], sys.argv[3]
f = lib.adanerf_host_pack_weights
f.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int32)]
lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
rng = np.random.default_rng(0)
codes = {}
for it in range(240):
    if os.path.exists(work): shutil.rmtree(work)
    shutil.copytree(src, work)
    name = ["model0.onnx", "model1.onnx", "config.ini", "dataset_info.txt"][it % 4]
    path = os.path.join(work, name)
    b = bytearray(open(path, "rb").read())
    mode = (it // 4) % 4
    if mode == 0: b = b[:int(rng.integers(0, len(b)))]                                   # truncation
    elif mode == 1:
        for _ in range(int(rng.integers(1, 40))): b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))   # byte flips
    elif mode == 2: b = bytearray(rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8).tobytes())   # garbage
    else:                                                                                 # flips confined to the first 4 KiB (headers)
        for _ in range(int(rng.integers(1, 20))): b[int(rng.integers(0, min(len(b), 4096)))] = int(rng.integers(0, 256))
    open(path, "wb").write(bytes(b))
    o = R._Options(width=32, height=24, batch_rays=-1, precision=0, threshold=-1.0, shard_world=1)
    info = R.Info()
    rc1 = lib.adanerf_host_parse_model(work.encode(), C.byref(o), C.byref(info))
    wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    rc2 = f(work.encode(), it % 2, 0, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
    if rc2 == 0 and wb.value < (1 << 28):
        w = np.empty(wb.value, np.uint8); bb = np.empty(bf.value, np.float32); lay = np.empty((nl.value, 4), np.int32)
        rc2 = f(work.encode(), it % 2, 0, w.ctypes.data, C.byref(wb), bb.ctypes.data, C.byref(bf), lay.ctypes.data, C.byref(nl))
    codes[(rc1, rc2)] = codes.get((rc1, rc2), 0) + 1
    assert rc1 in (0, -1, -2, -4) and rc2 in (0, -1, -2, -4), (name, mode, rc1, rc2)
print("OK", sorted(codes.items()))
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", script, root, d, str(tmp_path / "work")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK"), (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    assert "(-2," in out.stdout or ", -2)" in out.stdout      # corruption was actually detected in some cases


REF_SAMPLE_DIRS = {"sample_pavillon_16": "/root/reference/adanerf_real_time_viewer/sample_pavillon_16",
                   "sample": "/root/reference/adanerf_real_time_viewer/sample"}


@pytest.mark.skipif(not all(os.path.isdir(p) for p in REF_SAMPLE_DIRS.values()),
                    reason="the reference's shipped model directories exist in the build container only")
@pytest.mark.parametrize("tag", sorted(REF_SAMPLE_DIRS))
def test_cxx_loader_reads_the_reference_sample_dirs(lib, tmp_path, tag):
    """The drop-in claim at the file level: the C++ loader (format.cpp) is fed the reference's OWN exported model
    directories -- config.ini as src/export.py wrote it (the 71-line training form for `sample`, the trimmed 19-key form
    for `sample_pavillon_16`), dataset_info.txt, and the two torch.onnx.export files (Slice/Split/Gemm/Relu/Concat
    graphs, opset 9) -- and must (a) parse them to the scalars the oracle's independent reader finds, (b) pack every
    network / precision to exactly the bytes it packs from this repo's re-encoded weight fixture of the same model
    (tests/golden/weights_<tag>.npz written back through the minimal ONNX writer)."""
    src = REF_SAMPLE_DIRS[tag]
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    o = _opts(width=800, height=800)
    assert lib.adanerf_host_parse_model(src.encode(), C.byref(o), C.byref(info)) == 0, lib.adanerf_last_error(None)
    sc = O.load_scene(src + "/")
    assert info.num_samples == sc.num_samples and abs(info.threshold - sc.threshold) < 1e-7
    assert (info.n_in0, info.n_in1, info.use_ndc, info.dense) == (sc.n_in0, sc.n_in1, int(sc.use_ndc), 0)
    assert abs(info.fov - sc.fov) < 1e-6 and abs(info.max_depth - sc.max_depth) < 1e-5
    assert np.allclose([info.depth_range[0], info.depth_range[1]], sc.depth_range, rtol=1e-6)
    assert np.allclose(list(info.view_cell_center), sc.view_cell_center, rtol=1e-6)
    assert abs(info.view_cell_radius - sc.radius) < 1e-6
    assert info.sampler_mode == R.SAMPLER_ADAPTIVE
    # trailing separator optional (the viewer's CLI passes "model/")
    assert lib.adanerf_host_parse_model((src + "/").encode(), C.byref(o), C.byref(info)) == 0
    # the same weights through this repo's writer
    z = np.load(os.path.join(ROOT, "tests", "golden", "weights_%s.npz" % tag))
    wts = O.Weights({k[3:]: z[k] for k in z.files if k.startswith("n0/")}, {k[3:]: z[k] for k in z.files if k.startswith("n1/")})
    d, _, _ = _model_dir(tmp_path, sc, wts, name="re_" + tag)
    for net, precs in ((0, (2, 3, 1)), (1, (0, 1, 2))):
        for prec in precs:
            a = pack_weights(lib, src, net, prec)
            b = pack_weights(lib, d, net, prec)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y), (tag, net, prec)
    # depth table from the shipped dataset_info.txt
    lib.adanerf_host_depth_table.argtypes = [C.c_char_p, C.POINTER(R._Options), C.c_void_p]
    zt = np.zeros(128, dtype=np.float32)
    assert lib.adanerf_host_depth_table(src.encode(), C.byref(o), zt.ctypes.data) == 0
    np.testing.assert_allclose(zt, O.to_world_depth(O.bin_t(np.arange(128)), sc), rtol=3e-7, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# SURVEY 8f N3 (input handling half): the viewer's InputHandler / Camera movement, replayed from a script without a device
# ---------------------------------------------------------------------------------------------

def replay_reference_input(script, centre, size, n_batches):
    """What adanerf_real_time_viewer does with these events, restated in float32 numpy:
    inputhandler.cpp:19-104 (W/A/S/D/Q/E start / stop movement, O toggles the sampling-network view on key-up, ESC quits,
    left-button drag -> Camera::MouseDrag), camera.cpp:47-49, 90-91 (speed_mult = max(view_cell_size / 2), start at the
    view-cell centre with yaw -80, pitch 0), :128-141 (0.15 deg per pixel, pitch clamped to +-89), :143-158 (dir from
    yaw / pitch, right = dir x (0,0,1) and up = right x dir, neither normalised), :160-185 (one step of
    0.005 * speed_mult per axis and BATCH)."""
    f32 = np.float32
    pos = np.array(centre, f32)
    yaw, pitch = f32(-80.0), f32(0.0)
    speed = f32(0.005) * f32(max(s / 2 for s in size))
    mv = dict(fwd=0, right=0, up=0)
    keymap = dict(w=("fwd", 1), s=("fwd", -1), a=("right", -1), d=("right", 1), q=("up", 1), e=("up", -1))
    left, last, oracle, log = False, (0, 0), False, []
    for line in script:
        tok = line.split("#")[0].split()
        i = 0
        quit_ = False
        while i < len(tok):
            t = tok[i]
            if t in ("b+", "b-", "m"):
                x, y = int(tok[i + 1]), int(tok[i + 2])
                i += 3
                if t == "b+":
                    left, last = True, (x, y)
                elif t == "b-":
                    left = False
                else:
                    if left and (x, y) != last:
                        yaw = f32(yaw - f32(x - last[0]) * f32(0.15))
                        pitch = f32(np.clip(f32(pitch - f32(y - last[1]) * f32(0.15)), -89.0, 89.0))
                    last = (x, y)
                continue
            i += 1
            name = t[1:]
            if name in keymap:
                axis, sign = keymap[name]
                mv[axis] = sign if t[0] == "+" else 0
            elif t == "-o":
                oracle = not oracle
            elif t == "-esc":
                quit_ = True
        if quit_:
            break
        deg = f32(0.017453292519943295)
        d = np.array([np.cos(yaw * deg) * np.cos(pitch * deg), np.sin(yaw * deg) * np.cos(pitch * deg), np.sin(pitch * deg)], f32)
        d = (d / np.sqrt((d * d).sum(dtype=f32))).astype(f32)
        r = np.array([d[1], -d[0], 0], f32)
        u = np.cross(r, d).astype(f32)
        for _ in range(n_batches):
            for vec, k in ((d, "fwd"), (r, "right"), (u, "up")):
                if mv[k]:
                    pos = (pos + vec * speed * f32(mv[k])).astype(f32)
        log.append((pos.copy(), float(yaw), float(pitch), oracle))
    return log


INPUT_SCRIPT = ["+w", "", "-w +d", "b+ 100 100", "m 140 90", "m 150 40   # still dragging", "b- 150 40 -d", "m 10 10", "-o", "+q +s",
                "-q -o", "+e", "-e -s +a", "b+ 0 0 m 0 -700", "-a b- 0 0", "-esc", "+w"]


@pytest.mark.parametrize("n_batches", [1, 3])
def test_input_replay_moves_the_camera_like_the_viewer(tmp_path, n_batches):
    import subprocess
    from adanerf_amd import build as B
    exe = B.build_cli()
    z, meta, sc = load_case("classroom_n8_thr02")
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, case_weights(meta))
    script = tmp_path / "input.txt"
    script.write_text("\n".join(INPUT_SCRIPT) + "\n")
    out = subprocess.run([exe, md, "-s", "60", "40", "-nb", str(n_batches), "--script", str(script), "--log-camera", "--dry-run"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
    want = replay_reference_input(INPUT_SCRIPT, sc.view_cell_center, sc.view_cell_size, n_batches)
    assert len(got) == len(want) == 15                         # the ESC line ends the session, the line behind it never runs
    for g, (pos, yaw, pitch, oracle) in zip(got, want):
        np.testing.assert_allclose([float(g[3]), float(g[4]), float(g[5])], pos, rtol=0, atol=2e-6)
        assert abs(float(g[7]) - yaw) < 1e-4 and abs(float(g[9]) - pitch) < 1e-4
        assert g[11] == ("oracle" if oracle else "image")
    assert want[13][2] == 89.0 and float(got[13][9]) == 89.0      # the 700-pixel drag runs into the pitch clamp
    assert any(w[3] for w in want) and not want[-1][3]
    bad = subprocess.run([exe, md, "--script", str(script), "--dry-run", "--log-camera", "-s", "8", "8", "--frames", "1", "--bogus"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0
    script.write_text("+w\n+zz\n")
    bad = subprocess.run([exe, md, "-s", "8", "8", "--script", str(script), "--dry-run"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "malformed script line 2" in bad.stdout


def test_coarse_fine_model_directory_parses(lib, tmp_path):
    """inFeatures [RayMarchFromPoses, RayMarchFromCoarse] (vanilla NeRF) is a supported model directory; what is
    not supported about it is said, not guessed."""
    import dataclasses
    from conftest import COARSE_FINE_CASES
    z, meta, sc = load_case(COARSE_FINE_CASES[0])
    wts = case_weights(meta)
    d = str(tmp_path / "cf")
    O.write_model_dir(d, sc, wts)
    info = R.Info()
    opt = R._Options(width=80, height=60, batch_rays=-1, threshold=-1.0, shard_world=1)
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(opt), C.byref(info)) == 0, lib.adanerf_last_error(None)
    assert info.sampler_mode == R.SAMPLER_COARSE_FINE and info.num_samples_coarse == 16 and info.num_samples == 40 and info.n_in0 == 90
    # model0.onnx packs as a NeRF net (the shading-net layout), for every precision
    for prec in (0, 1, 2):
        wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        assert lib.adanerf_host_pack_weights(d.encode(), 1, prec, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl)) == 0
        assert wb.value > 0 and nl.value == 11 + (1 if prec == 0 else 0)      # bf16: + the scaled packing's output exponents
    for key, val, msg in [("rayMarchSampler", "[UnitSphereLinearOutsideLog, none]", "LinearlySpacedZNearZFar"),
                          ("numRaymarchSamples", "[2, 8]", "3..128"), ("numRaymarchSamples", "[64, 2000]", "1024")]:
        bad = str(tmp_path / ("cf_bad_" + key + str(len(val))))
        O.write_model_dir(bad, sc, wts)
        ini = open(os.path.join(bad, "config.ini")).read()
        ini = re.sub(r"^%s = .*$" % key, "%s = %s" % (key, val), ini, flags=re.M)
        open(os.path.join(bad, "config.ini"), "w").write(ini)
        rc = lib.adanerf_host_parse_model(bad.encode(), C.byref(opt), C.byref(info))
        assert rc != 0 and msg in lib.adanerf_last_error(None).decode(), (key, val, lib.adanerf_last_error(None))


def test_bench_flop_models_match_the_survey_figures():
    """bench.py's algorithmic-FLOP models (the numerators of `roofline.achieved` / `sampling_roofline`): SURVEY 8d's 1 186 816 FLOP per
    shading sample and 898 048 per ray for the 8 x 256 networks, and the general-topology formula reproduces the first at L x W = 8 x 256."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.SHADE_FLOP_PER_SAMPLE == 2 * (63 * 256 + 4 * 256 ** 2 + 319 * 256 + 2 * 256 ** 2 + 256 + 256 ** 2 + 283 * 128 + 128 * 3) == 1186816
    assert bench.SAMPLE_FLOP_PER_RAY == 2 * (90 * 256 + 6 * 256 ** 2 + 256 * 128) == 898048
    assert bench.generic_shape("generic_6x128_random_init") == (6, 128, 2) and bench.generic_shape("classroom") is None
    assert bench.shade_flop_per_sample("generic_8x256_random_init") == bench.SHADE_FLOP_PER_SAMPLE
    w, d = 128, 6
    assert bench.shade_flop_per_sample("generic_6x128_random_init") == 2 * (63 * w + (d - 2) * w * w + (w + 63) * w + w * w + w + (w + 27) * (w // 2) + (w // 2) * 3)


def test_bench_watchdog_prints_the_line_it_has(tmp_path):
    """bench.py's Watchdog: a run stuck in a collective still ends with ONE JSON line from rank 0 -- the finished record if there is one (exit 0), else a
    line with value null and the reason (exit 3; a render-only fall-back record keeps its null value: phase A's rate is not an N-GPU frames/s); ranks other
    than 0 leave quietly.  Every phase gets the full time: setting `phase` re-arms the timer (a slow build does not eat the exchange's time)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "d = bench.Watchdog(0.6, int(sys.argv[1])); d.phase = 'exchange pre-flight (gather)'\n"
            "if sys.argv[2] == 'fallback': d.fallback = {'value': None, 'render_only': {'value': 5.0}, 'config': {'exchange': {'error': None}}}\n"
            "if sys.argv[2] == 'record': d.record = {'value': 7.0, 'config': {}}\n"
            "if sys.argv[2] == 'phases':\n"
            "    for k in range(5): time.sleep(0.4); d.phase = 'phase %%d' %% k\n"
            "    d.cancel(); print('survived'); sys.exit(0)\n"
            "time.sleep(5); print('not reached')\n") % root
    def run(rank, what):
        return subprocess.run([sys.executable, "-c", prog, str(rank), what], capture_output=True, text=True, timeout=60)
    a = run(0, "fallback")
    rec = json.loads(a.stdout.strip())
    assert a.returncode == 3 and rec["value"] is None and rec["render_only"]["value"] == 5.0 and "exchange pre-flight (gather)" in rec["config"]["exchange"]["error"] \
        and "watchdog" in rec["error"]
    b = run(0, "record")
    rec = json.loads(b.stdout.strip())
    assert b.returncode == 0 and rec["value"] == 7.0 and "watchdog" in rec["notes"][0]
    c = run(0, "nothing")
    assert c.returncode == 3 and json.loads(c.stdout.strip())["value"] is None
    d = run(1, "fallback")
    assert d.returncode == 0 and d.stdout.strip() == ""
    e = run(0, "phases")      # 5 x 0.4 s of progress under a 0.6 s per-phase limit
    assert e.returncode == 0 and e.stdout.strip() == "survived"


def test_bench_gpu_telemetry_degrades_without_a_gpu():
    """bench.py's GpuTelemetry (shader clock / socket power through librocm_smi64) is optional equipment: without a device, or without the library, it
    reports nulls with the reason and never raises or hangs (its thread is a daemon, its join is bounded)."""
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    t = bench.GpuTelemetry(0, period=0.01).start()
    time.sleep(0.05)
    rec = t.stop()
    assert set(rec) >= {"sclk_mhz_mean", "power_w_mean"}
    if rec["sclk_mhz_mean"] is None:
        assert rec.get("error") or rec.get("samples") is not None


def test_bf16_scaling_bound_refuses_scenes_beyond_it(lib, tmp_path):
    """bf16 shading nets are packed with per-layer powers of two derived from activation bounds that assume encoding inputs below
    kPosIdentityBound = 4096 (pack.hpp): a scene whose un-normalised sample positions can exceed that is refused for bf16 with a message
    (never clamped silently) and still loads for fp16; the shipped scenes are far inside."""
    import dataclasses
    sc = O.Scene((0.5, -1.0, 1.25), (0.7, 0.7, 0.2), (0.15, 8.25), 1.125, 8.75, 8, 0.2)
    far = dataclasses.replace(sc, view_cell_center=(9000.0, 0.0, 0.0), normalization="None")
    wts = O.synthetic_weights(3)
    info = R.Info()
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    for k, (scene, prec, ok) in enumerate([(sc, R.PREC_BF16, True), (far, R.PREC_BF16, False), (far, R.PREC_FP16, True),
                                           (dataclasses.replace(far, normalization="Centered"), R.PREC_BF16, True)]):
        d, _, _ = _model_dir(tmp_path, scene, wts, name="bound%d" % k)
        rc = lib.adanerf_host_parse_model(d.encode(), C.byref(_opts(precision=prec)), C.byref(info))
        assert (rc == 0) == ok, (k, rc, lib.adanerf_last_error(None))
        if not ok:
            assert rc == -4 and b"kPosIdentityBound" in lib.adanerf_last_error(None)


def test_scaled_bf16_packing_is_exact(lib, tmp_path):
    """The bf16 shading net is packed with per-layer powers of two (pack.cpp scale_layer) so that the kernels' ReLU is a clamped conversion.
    Powers of two commute with every rounding of the dataflow: the numpy replay of the scaled blob, un-scaled at its two outputs, equals the
    replay of the unscaled blob (host hook precision 4) BIT FOR BIT -- for the shipped 8 x 256 network and for run-time-shaped topologies --
    and no scaled ReLU output exceeds 1 (asserted inside the replay)."""
    rng = np.random.default_rng(5)
    z, meta, sc = load_case("classroom_n8_thr02")
    cases = [(case_weights(meta), "classroom", None)]
    for seed, layers, widths, skip in ((11, (8, 6), (256, 128), 2), (12, (8, 4), (256, 64), 1), (13, (8, 5), (256, 256), [0, 2])):
        cases.append((O.synthetic_weights(seed, layers=layers, widths=widths, skip1=skip), "syn%d" % seed, (layers[1], widths[1])))
    n = 64
    x = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for wts, name, shape in cases:
        md, _, _ = _model_dir(tmp_path, sc, wts, name="scaled_" + name)
        ws, bs, ls = pack_weights(lib, md, 1, 0)
        wu, bu, lu = pack_weights(lib, md, 1, 4)
        assert int(ls[-1][3]) == -1 and int(lu[-1][3]) != -1 and ws.size == wu.size and not np.array_equal(ws, wu)
        ns, nu = PackedNet(ws, bs, ls, 0), PackedNet(wu, bu, lu, 0)
        assert ns.scaled and not nu.scaled
        if shape is None:
            a, b = run_shading_net(ns, x, d), run_shading_net(nu, x, d)
        else:
            depth, skips = O.shading_topology(wts.net1, 63)
            a, b = (run_shading_net_generic(q, x, d, depth, pad_to(shape[1]), skips) for q in (ns, nu))
        assert np.isfinite(a).all() and np.array_equal(a, b), (name, float(np.abs(a - b).max()))
        assert 0.0 < ns.max_relu_out <= 1.0


def test_scaled_bf16_packing_refuses_a_bound_beyond_its_range(lib, tmp_path):
    """pack.cpp scale_layer: the per-layer activation bound is a product of L1 row norms and is loose by construction; when it leaves 2^100 the
    scaled packing can prove nothing about what the clamped conversion would cut, so a bf16 shading net like that is REFUSED with a message (it used
    to clamp the exponent silently: ADVICE round 5) -- the same network still packs for fp16 and unscaled (host hook precision 4)."""
    z, meta, sc = load_case("classroom_n8_thr02")
    wts = O.synthetic_weights(21)
    big = {k: (v * np.float32(3.0e4) if k.startswith("pts_linears.") and k.endswith(".weight") else v) for k, v in wts.net1.items()}
    import dataclasses
    md, _, _ = _model_dir(tmp_path, sc, dataclasses.replace(wts, net1=big), name="hugebound")
    f = lib.adanerf_host_pack_weights
    f.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int32)]
    f.restype = C.c_int
    wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    rc = f(md.encode(), 1, 0, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
    assert rc != 0 and b"activation bound" in lib.adanerf_last_error(None) and b"pts_linears." in lib.adanerf_last_error(None), lib.adanerf_last_error(None)
    for prec in (1, 4):      # fp16; bf16 without the scaling
        assert f(md.encode(), 1, prec, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl)) == 0, lib.adanerf_last_error(None)


def pad_to(w):
    return 64 if w <= 64 else 128 if w <= 128 else 256


# ---- the host-side loader on damaged and hostile model directories (round 6) ---------------------------------------------------

def _pb_varint(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v > 0x7F else 0))
        v >>= 7
        if not v:
            return bytes(out)


def _pb_bytes(num, payload):
    return bytes([(num << 3) | 2]) + _pb_varint(len(payload)) + payload


def _crafted_onnx(name, dims, raw=b""):
    """ModelProto{graph{initializer{dims..., data_type FLOAT, name, raw_data}}} as torch.onnx.export writes them (format.cpp's wire reader)."""
    t = b"".join(bytes([1 << 3]) + _pb_varint(d) for d in dims) + bytes([2 << 3, 1]) + _pb_bytes(8, name.encode()) + _pb_bytes(9, raw)
    return _pb_bytes(7, _pb_bytes(5, t))


def test_crafted_initializers_are_refused_through_the_c_abi(lib, tmp_path):
    """A model0.onnx whose tensor dimensions wrap (int(2^31) x int(2^31) elements x 4 bytes = 0 = the empty raw_data), are negative as
    int32 or exceed what the file can hold used to reach std::vector::resize with 2^62 elements -- an exception through the C ABI ends the host
    process.  Now: refused as malformed, and no loader exception leaves adanerf_host_* / adanerf_create (they return ADANERF_EIO + message)."""
    f = lib.adanerf_host_pack_weights
    f.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int32)]
    f.restype = C.c_int
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    d, _, _ = _model_dir(tmp_path, name="crafted")
    good = open(os.path.join(d, "model0.onnx"), "rb").read()
    M = 1 << 31
    for dims, raw in (((M, M), b""), ((0xFFFFFFFF, 4), b""), ((1 << 30, 1 << 30, 4), b""), ((2, 3), b"\0" * 8), (((1 << 64) - 1,), b"")):
        with open(os.path.join(d, "model0.onnx"), "wb") as fh:
            fh.write(_crafted_onnx("layers.0.weight", dims, raw))
        wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        rc = f(d.encode(), 0, 0, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
        assert rc != 0 and b"malformed ONNX" in lib.adanerf_last_error(None), (dims, rc, lib.adanerf_last_error(None))
    # a band count no int can hold (the callers convert posEncArgs to int) is refused by the range check, not converted
    with open(os.path.join(d, "model0.onnx"), "wb") as fh:
        fh.write(good)
    cfg = open(os.path.join(d, "config.ini")).read()
    assert "posEncArgs" in cfg
    import re
    for bad in ("1e39-4", "nan-4", "10-99999999999"):
        with open(os.path.join(d, "config.ini"), "w") as fh:
            fh.write(re.sub(r"posEncArgs\s*=.*", "posEncArgs = [%s, 10-4]" % bad, cfg))
        info, o = R.Info(), _opts()
        rc = lib.adanerf_host_parse_model(d.encode(), C.byref(o), C.byref(info))
        assert rc != 0 and b"posEncArgs" in lib.adanerf_last_error(None), (bad, rc, lib.adanerf_last_error(None))


def test_host_loader_under_sanitizers_on_mutated_model_directories(tmp_path):
    """tests/host_sanitize_fuzz.cpp: format.cpp + pack.cpp built with g++ -fsanitize=address,undefined,float-cast-overflow and run on crafted
    initializers, 76 well-formed files of odd topologies and 150 randomly damaged model directories.  Any outcome but a fault is fine."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    from adanerf_amd.build import CSRC
    exe = str(tmp_path / "host_sanitize_fuzz")
    san = "-fsanitize=address,undefined,float-cast-overflow"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", san, "-fno-sanitize-recover=undefined,float-cast-overflow", "-I", CSRC,
           os.path.join(ROOT, "tests", "host_sanitize_fuzz.cpp"), os.path.join(CSRC, "format.cpp"), os.path.join(CSRC, "pack.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "error:" not in built.stderr.replace("ld: error", ""):
        pytest.skip("sanitizer runtimes not installed: " + built.stderr[-200:])
    assert built.returncode == 0, built.stderr[-2000:]
    d, _, _ = _model_dir(tmp_path, name="fuzzed")
    work = tmp_path / "work"
    work.mkdir()
    out = subprocess.run([exe, d, str(work), "150", "606"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "0 faults" in out.stdout, out.stdout[-500:] + out.stderr[-3000:]


def test_host_only_entry_points_under_sanitizers(tmp_path):
    """tools/host_abi_sanitize.sh: the library's own host code (the three .hip translation units compiled --cuda-host-only, the five .cpp ones as they are)
    with -fsanitize=address,undefined, and adanerf_host_parse_model / _depth_table / _pack_weights called through the C ABI on 200 randomly
    damaged model directories (tests/host_abi_fuzz.cpp).  Covers what the g++ harness above cannot: setup_model (csrc/model_setup.cpp), i.e. every check
    adanerf_create makes on config.ini / dataset_info.txt, and the shape adanerf_host_pack_weights derives from them (round 6: a saturated
    raySampleInput overflowed an int in the packer there)."""
    import shutil
    import subprocess
    if not shutil.which("hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("hipcc / clang++ not available")
    import glob
    if not glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.*"):
        pytest.skip("clang sanitizer runtimes not installed")
    out_dir = str(tmp_path / "audit")
    built = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_abi_sanitize.sh"), out_dir], capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stdout[-1000:] + built.stderr[-3000:]
    d, _, _ = _model_dir(tmp_path, name="abi_fuzzed")
    work = tmp_path / "work_abi"
    work.mkdir()
    out = subprocess.run([os.path.join(out_dir, "host_abi_fuzz"), d, str(work), "200", "707"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "0 faults" in out.stdout and "untouched: 10 calls ok" in out.stdout, out.stdout[-500:] + out.stderr[-3000:]
