"""What the pre-DAS stage tests share: the cases, the push that captures the DAS input, the oracle's run of the same plan, the
element-wise bounds, and the Hilbert stage's acquisitions and fixture.  Imports tests/das_push.py and no test module."""
import ctypes as C
import math

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P
from tests.das_push import compare


S = P.ShaderKind
DK = P.DataKind
U32 = 2.0 ** -24          # unit roundoff of binary32
U16 = 2.0 ** -11          # ... of binary16
# An input sample that the shader rounds to binary16 after the demodulation rotation may land one binary16 ulp (2 u) apart in
# the two builds (the GPU contracts c*x - s*y to an FMA, the oracle does not), and the scale multiply that follows may round
# the other way once more (2 u): 4 u per sample, taken as 6 u for the ulp at a binade edge.
K_SAMPLE = 6
# Binary16 store of a stage output: one rounding of values already within the propagated bound of each other.
K_STORE = 2
# Int16 / Int16Complex store of a stage output: a truncation toward zero (stages.hip store_scalar, GLSL's int16_t(v)).  Two
# evaluations within e of each other store integers within e + 1 -- |trunc(a) - trunc(b)| < |a - b| + 1 -- so the store adds 1, in the
# stored unit, to the bar.  Derived, not measured.  Where the value stored is an exactly computed integer (a Reshape's copy, a Decode
# of exact integers: partial sums below 2^24, one identical division) both builds truncate the same number and nothing is added.
I16_STORE = 1.0
# ... and a float outside the int16 range converts differently on host and device: every Int16-stored stage's magnitude bound
# stays below half the range (the cases divide their Int16 RF by 8 for it)
I16_RANGE = 16384.0


def k_sum(n):
    """Two recursive sums of n products, each within gamma_{n+1} = (n+1) u of the exact sum (Higham 3.1): 2 (n + 1)."""
    return 2 * (n + 1)


def filter_taps(oracle, fp, real_samples=False):
    """(magnitude per tap |hr| + |hi| or |h|, length, complex_filter) exactly as both builds read the taps (Q7: complex taps only
    for a matched chirp).  real_samples: the stage filters real samples without demodulating them -- of complex taps only the real
    parts enter (filter.glsl's real SAMPLE_TYPE reads coefficients[2 j]), so the magnitude per tap is |hr|."""
    from oracle.binding import library
    buf = np.zeros(8192, np.float32)
    delay = C.c_float(0)
    L = library().oracle_filter_create(C.byref(fp), buf.ctypes.data_as(C.POINTER(C.c_float)), 8192, C.byref(delay))
    assert L > 0
    complex_filter = bool(fp.complex) and fp.kind == int(P.FilterKind.MatchedChirp)
    if complex_filter and real_samples:
        h = np.abs(buf[0:2 * L:2].astype(np.float64))
    elif complex_filter:
        h = np.abs(buf[0:2 * L:2].astype(np.float64)) + np.abs(buf[1:2 * L:2].astype(np.float64))
    else:
        h = np.abs(buf[:L].astype(np.float64))
    return h, L, complex_filter


def hilbert_taps(oracle):
    """(|hr| + |hi| per tap, length) of the build-defined Hilbert FIR, in the correlation order both builds apply it"""
    taps = np.zeros(2 * 63, np.float32)
    oracle.library().oracle_hilbert_fir(taps.ctypes.data_as(C.POINTER(C.c_float)))
    return np.abs(taps[0::2].astype(np.float64)) + np.abs(taps[1::2].astype(np.float64)), 63


def plan_of(bflib, acq):
    L = bflib.library()
    for slot, fp in enumerate(acq.filters):
        assert L.beamformer_create_filter(C.byref(fp), slot, 0)
    assert L.beamformer_push_simple_parameters(C.byref(acq.bp))
    plan = P.HipPlan()
    assert L.beamformer_hip_describe_plan(0, C.byref(plan))
    return plan


def mapped_rf_magnitudes(acq):
    """|scalar| of the RF slot after ingest (channel map, A1S2 contrast, raw padding dropped), flat, float64"""
    bp = acq.bp
    Cn, A, Sn = int(bp.channel_count), int(bp.acquisition_count), int(bp.sample_count)
    n_scalar = 2 if P.DATA_KIND_COMPLEX[int(bp.data_kind)] else 1
    raw = np.abs(np.asarray(acq.rf).reshape(int(bp.raw_data_dimensions[1]), -1).astype(np.float64))
    rows = raw[[int(bp.channel_mapping[c]) for c in range(Cn)]]
    row = A * Sn * n_scalar
    if bp.contrast_mode:
        n = Sn * n_scalar
        out = np.zeros((Cn, row))
        out[:, :n] = rows[:, :n] + rows[:, n:2 * n] + rows[:, 2 * n:3 * n]
        return out.reshape(-1)
    return rows[:, :row].reshape(-1)


def stage_bounds(bflib, oracle, acq, plan, trace=None):
    """Walks the library's plan over scalar buffers and returns (exact, magnitude, bar) of the DAS input, both (C, A, Sd)
    arrays: `magnitude` bounds |value| (|re| + |im| for complex), `bar` the distance two faithful evaluations can have.
    exact: every stage on the way is exact arithmetic (then the comparison is bit-identical)."""
    bp = acq.bp
    Cn, A = int(bp.channel_count), int(bp.acquisition_count)
    Sd = int(plan.das_samples)
    mag = mapped_rf_magnitudes(acq)
    err = np.zeros_like(mag)
    exact, integer = True, P.DATA_KIND_NUMPY[int(bp.data_kind)] == "int16"
    n_ch = np.arange(Cn)[:, None, None]
    n_tx = np.arange(A)[None, :, None]
    n_s = np.arange(Sd)[None, None, :]

    def elements(buf, kind):
        return buf[0::2] + buf[1::2] if kind & 1 else buf

    def scatter(size_elements, kind, index, values_mag, values_err):
        # A complex element's magnitude and error are bounds on |re| + |im| and on |d re| + |d im|: with taps h = hr + i hi,
        # |out re| + |out im| <= sum (|hr| + |hi|) (|x re| + |x im|), and a real operation (Decode, real taps) keeps the two parts apart.
        # Each of the element's two scalars holds half of the bound, so that `elements` returns it -- not twice it -- to the next
        # stage; one scalar alone is bounded by the element's whole bound, which is what the DAS input is judged by below.
        n = 2 if kind & 1 else 1
        m = np.zeros(size_elements * n)
        e = np.zeros(size_elements * n)
        for k in range(n):
            m[n * index + k] = values_mag / n
            e[n * index + k] = values_err / n
        return m, e

    kinds = [int(plan.stages[i].kind) for i in range(plan.stage_count)]
    das_index = kinds.index(int(S.DAS))
    # the filter slot of every stage comes from the oracle's plan (the library's describe call does not carry it): first the two plans
    # must list the same stages, as tests/test_host_logic.py's test_planner_agrees_with_oracle asks of the named cases
    ref_plan = oracle.plan(bp, acq.filters)
    assert ref_plan is not None, "the oracle cannot plan this pipeline"
    assert [int(ref_plan.stages[i].kind) for i in range(ref_plan.stage_count)] == kinds, "the library's and the oracle's plans list different stages"
    for i in range(das_index):
        st = plan.stages[i]
        kind = int(st.kind)
        assert (int(ref_plan.stages[i].in_kind), int(ref_plan.stages[i].out_kind)) == (int(st.in_kind), int(st.out_kind)), (i, kind)
        ist, ost = [int(v) for v in st.in_stride], [int(v) for v in st.out_stride]
        in_m, in_e = elements(mag, st.in_kind), elements(err, st.in_kind)
        out_f16 = (st.out_kind >> 1) == 2
        out_i16, in_i16 = (st.out_kind >> 1) == 0, (st.in_kind >> 1) == 0
        if kind == int(S.Reshape):
            assert not (not (st.in_kind & 1) and (st.out_kind & 1)), "interleaving Reshape: not modelled"
            src = ist[0] * n_s + ist[1] * n_ch + ist[2] * n_tx
            dst = ost[0] * n_s + ost[1] * n_ch + ost[2] * n_tx
            if out_f16 and not integer:
                exact = False
            # past the end of its input a Reshape reads zeros, as the filters do (in_elements; a Decode-first pipeline that also
            # demodulates walks the RF with the root's strides in complex elements, twice the RF's length)
            inside = src < len(in_m)
            src_m = np.where(inside, in_m[np.minimum(src, len(in_m) - 1)], 0.0)
            src_e = np.where(inside, in_e[np.minimum(src, len(in_m) - 1)], 0.0)
            store = K_STORE * U16 * src_m if out_f16 else 0
            if out_i16 and not in_i16:                                      # a converting Reshape truncates; Int16 -> Int16 copies
                assert src_m.max() < I16_RANGE, f"stage {i}: Int16 store of magnitudes up to {src_m.max():.0f}"
                exact, store = False, I16_STORE * (2 if st.out_kind & 1 else 1)
            mag, err = scatter(int(dst.max()) + 1, st.out_kind, dst, src_m, src_e + store)
        elif kind == int(S.Decode):
            T = A
            src = ((n_s * Cn + n_ch) * T)[:, 0, :]                          # (C, Sd): element j at + j (decode kernel layout)
            M = sum(in_m[src + j] for j in range(T)) / T
            E = sum(in_e[src + j] for j in range(T)) / T
            if not integer:                                                 # integer partial sums: exact, one identical division
                exact = False
                E = E + k_sum(T) * (U16 if out_f16 else U32) * M
                if out_i16:
                    E = E + I16_STORE * (2 if st.out_kind & 1 else 1)
            if out_i16:
                assert M.max() < I16_RANGE, f"stage {i}: Int16 store of magnitudes up to {M.max():.0f}"
            # an exact Decode stored as Int16 holds exactly computed integers again (both builds truncate the one quotient)
            integer = integer and out_i16
            dst = ost[0] * n_s + ost[1] * n_ch + ost[2] * n_tx
            mag, err = scatter(int(dst.max()) + 1, st.out_kind, dst, np.broadcast_to(M[:, None, :], dst.shape),
                               np.broadcast_to(E[:, None, :], dst.shape))
        elif kind in (int(S.Filter), int(S.Demodulate)):
            demod = kind == int(S.Demodulate)
            slot = int(ref_plan.stages[i].filter_slot) % P.FILTER_SLOTS
            assert slot < len(acq.filters) and acq.filters[slot] is not None, f"stage {i} reads filter slot {slot}: the case sets none"
            h, L, complex_filter = filter_taps(oracle, acq.filters[slot], real_samples=not demod and not st.in_kind & 1)
            D = max(1, int(bp.decimation_rate)) if demod else 1
            f16 = (st.in_kind >> 1) != 1
            scale = 1.0
            if demod:
                # the rotation keeps |s| but may grow |re| + |im| by sqrt(2); times the shader's scale (filter.glsl:98)
                scale = math.sqrt(2.0) * (1.0 + 2 * U16)
                if not complex_filter:
                    scale *= float(np.float16(math.sqrt(2.0))) if f16 else float(np.float32(math.sqrt(2.0)))
            terms = 2 * L if complex_filter and (demod or st.in_kind & 1) else L
            keep = Sd // D
            M = np.zeros((Cn, A, Sd))
            E = np.zeros((Cn, A, Sd))
            n_el = len(in_m)
            for c in range(Cn):
                for t in range(A):
                    row_start = ist[1] * c + ist[2] * t
                    if demod:
                        row_start //= 2                                     # filter.glsl:81-87 (non-negative: floor = truncation)
                    lo = row_start - (L - 1)
                    hi = row_start + D * (keep - 1) + 1
                    idx = np.arange(lo, hi)
                    ok = (idx >= 0) & (idx < n_el)
                    seg_m = np.where(ok, in_m[np.clip(idx, 0, n_el - 1)], 0.0)
                    seg_e = np.where(ok, in_e[np.clip(idx, 0, n_el - 1)], 0.0)
                    M[c, t, :keep] = scale * np.correlate(seg_m, h, "valid")[::D][:keep]
                    E[c, t, :keep] = scale * np.correlate(seg_e, h, "valid")[::D][:keep]
                    # filter.glsl:79: a 64-output group whose window would start before its row (D x group x 64 < L - 1) reads zeros
                    # for the window's first L - 1 entries -- not what lies in front of the row start.  The bound follows: a row that
                    # starts inside the buffer (decode layout, a halved row start) takes nothing from the elements before it there
                    for wg in range((keep + 63) // 64):
                        if D * wg * 64 >= L - 1:
                            break
                        front = idx < row_start + D * wg * 64
                        group = slice(wg * 64, min(keep, wg * 64 + 64))
                        M[c, t, group] = scale * np.correlate(np.where(front, 0.0, seg_m), h, "valid")[::D][group]
                        E[c, t, group] = scale * np.correlate(np.where(front, 0.0, seg_e), h, "valid")[::D][group]
            u_in = U16 if f16 else U32
            E = E + ((K_SAMPLE * u_in if demod else 0.0) + k_sum(terms) * U32) * M
            if out_f16:
                E = E + K_STORE * U16 * M
            if out_i16:
                assert M.max() < I16_RANGE, f"stage {i}: Int16 store of magnitudes up to {M.max():.0f}"
                E = E + I16_STORE * (2 if st.out_kind & 1 else 1)      # both scalars of a complex element truncate
            exact = integer = False
            dst = ost[0] * n_s + ost[1] * n_ch + ost[2] * n_tx
            if st.in_kind & 1 and not (st.out_kind & 1):                    # deinterleaving store: re, then im a batch later
                batch = Cn * Sd * A
                mag = np.zeros(2 * batch)
                err = np.zeros(2 * batch)
                for part in (0, batch):
                    mag[dst + part] = M
                    err[dst + part] = E
            else:
                mag, err = scatter(int(dst.max()) + 1, st.out_kind, dst, M, E)
        elif kind == int(S.Hilbert):
            # a filter stage without demodulation: 63 complex taps on the real input samples of the row itself (outside it: zero),
            # L terms per component, f32 products and sums; int / f16 -> f32 conversion of the input is exact
            assert not st.in_kind & 1 and st.out_kind & 1, "the Hilbert stage takes real samples and stores complex ones"
            h, L = hilbert_taps(oracle)
            M = np.zeros((Cn, A, Sd))
            E = np.zeros((Cn, A, Sd))
            pad = np.zeros(L - 1)
            for c in range(Cn):
                for t in range(A):
                    row = ist[0] * np.arange(Sd) + ist[1] * c + ist[2] * t
                    M[c, t] = np.correlate(np.concatenate([pad, in_m[row]]), h, "valid")
                    E[c, t] = np.correlate(np.concatenate([pad, in_e[row]]), h, "valid")
            E = E + k_sum(L) * U32 * M
            if out_f16:
                E = E + K_STORE * U16 * M
            exact = integer = False
            dst = ost[0] * n_s + ost[1] * n_ch + ost[2] * n_tx
            mag, err = scatter(int(dst.max()) + 1, st.out_kind, dst, M, E)
        else:
            raise AssertionError(f"stage kind {kind} not modelled")
        if trace is not None:                                               # (stage, out kind, median magnitude bound, median bar) of what it wrote
            live = mag > 0
            trace.append((kind, int(st.out_kind), float(np.median(mag[live])) if live.any() else 0.0, float(np.median(err[live])) if live.any() else 0.0))
    das = plan.stages[das_index]
    ist = [int(v) for v in das.in_stride]
    src = ist[0] * n_s + ist[1] * n_ch + ist[2] * n_tx
    return exact, elements(mag, das.in_kind)[src], elements(err, das.in_kind)[src]


def oracle_run(oracle, acq):
    captured = {}
    flags = {} if acq.bp.interpolation_mode == int(P.InterpolationMode.Nearest) else None
    ref, _ = oracle.beamform(acq.bp, acq.rf, acq.filters, flags=flags, das_input=captured)
    return ref, flags, captured["data"]


def push(bflib, acq, hooks=None, poison=True, mode=0):
    L = bflib.library()
    if hooks is not None:
        if poison:
            hooks.set("SCRATCH_POISON")
        else:
            hooks.clear("SCRATCH_POISON")
    L.beamformer_hip_set_das_path(mode)
    try:
        frame = bflib.beamform(acq.bp, acq.rf, acq.filters)
        das_input = bflib.das_input(acq.bp)
    finally:
        L.beamformer_hip_set_das_path(0)
    return frame, das_input


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def check_das_input(bflib, oracle, acq, gpu_in, ref_in, label=""):
    """the element-wise bar; returns ('bit-identical', 0) or ('bound', max err/bar)"""
    plan = plan_of(bflib, acq)
    assert gpu_in.shape == ref_in.shape, (gpu_in.shape, ref_in.shape)
    assert not np.isnan(ref_in).any(), "the oracle's DAS input holds NaN"
    nan = np.isnan(gpu_in)
    if nan.any():
        c, t, s = np.argwhere(nan)[0]
        raise AssertionError(f"{label}: {int(nan.sum())} DAS-input elements are NaN (read without having been written this frame), "
                             f"first at channel {c} transmit {t} sample {s} of {gpu_in.shape[2]} "
                             f"(decimation {acq.bp.decimation_rate}: samples [{gpu_in.shape[2] // max(1, acq.bp.decimation_rate)}, "
                             f"{gpu_in.shape[2]}) are the filter's tail)")
    exact, mag, bar = stage_bounds(bflib, oracle, acq, plan)
    if exact:
        diff = as_bits(gpu_in) != as_bits(ref_in)
        assert not diff.any(), (f"{label}: exact stages but {int(diff.sum())} DAS-input scalars differ in their bits, "
                                f"first at {np.argwhere(diff.reshape(gpu_in.shape + (-1,)) if np.iscomplexobj(gpu_in) else diff)[0]}")
        print(f"{label}: DAS input bit-identical")
        return "bit-identical", 0.0
    if np.iscomplexobj(gpu_in):
        err = np.maximum(np.abs(gpu_in.real.astype(np.float64) - ref_in.real), np.abs(gpu_in.imag.astype(np.float64) - ref_in.imag))
    else:
        err = np.abs(gpu_in.astype(np.float64) - ref_in)
    over = err > bar
    if over.any():
        c, t, s = np.argwhere(over)[0]
        raise AssertionError(f"{label}: {int(over.sum())} DAS-input elements outside the forward-error bound; first at channel {c} "
                             f"transmit {t} sample {s}: gpu {gpu_in[c, t, s]} oracle {ref_in[c, t, s]} bar {bar[c, t, s]:.3e}")
    live = bar > 0
    ratio = float((err[live] / bar[live]).max()) if live.any() else 0.0
    print(f"{label}: DAS input within the bound, max err/bar {ratio:.3e}")
    return "bound", ratio


def run_case(bflib, oracle, hooks, acq, modes=(0,)):
    ref, flags, ref_in = oracle_run(oracle, acq)
    results = []
    for mode in modes:
        gpu, gpu_in = push(bflib, acq, hooks, poison=True, mode=mode)
        results.append((gpu, gpu_in, check_das_input(bflib, oracle, acq, gpu_in, ref_in, f"{acq.name} mode {mode:#x}")))
        compare(gpu, ref, acq, flags)
    return ref, ref_in, results


FS, FD, PITCH = 25e6, 6.25e6, 0.3e-3


def deepest_sample(acq, plan):
    """the sample index of one in-aperture term at the deepest voxel on the image axis (x = 0): the transmit that reaches
    deepest, received on the element nearest the axis (das.glsl's plane-wave RCA geometry, as the oracle computes it)"""
    bp = acq.bp
    m = np.array(bp.das_voxel_transform[:], np.float64).reshape(4, 4).T
    z1 = (m @ np.array([0.5, 1.0, 0.0, 1.0]))[2] if bp.output_points[2] <= 1 else (m @ np.array([0.5, 0.5, 1.0, 1.0]))[2]
    half = (bp.channel_count - 1) / 2 * PITCH
    rx = min(math.hypot(c * PITCH - half, z1) for c in range(bp.channel_count))
    tx = max(z1 * math.cos(math.radians(bp.steering_angles[a])) for a in range(bp.acquisition_count))
    return ((tx + rx) / cfg.SPEED_OF_SOUND + plan.das_time_offset) * plan.das_sampling_frequency


def decimation_case(D, data_kind, L, A, decode, seed, C_=8, S_=2048, chirp=False):
    """{Demodulate, DAS} or {Demodulate, Decode, DAS} at decimation D, whose deepest voxels take terms from samples around
    1.4 Sd / D -- past the end of what the filter computes (Sd / D of the Sd samples of a DAS row)"""
    t_deep = 1.4 * (S_ / (2 * D * D)) / (FS / (2 * D))           # seconds: 1.4 x the first tail sample
    z1 = cfg.SPEED_OF_SOUND * t_deep / 2
    stages = (S.Demodulate, S.Decode, S.DAS) if decode else (S.Demodulate, S.DAS)
    name = f"dec{D}_{P.DataKind(data_kind).name}_L{L}_A{A}{'_decode' if decode else ''}{'_chirp' if chirp else ''}"
    acq = cfg.rca(name, C_, A, S_, (16, 1, 24), (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1), seed=seed, data_kind=data_kind,
                  demodulate=True, stages=stages, decimation=D, decode=1 if decode else 0, fs=FS, fd=FD, pitch=PITCH,
                  single=False, orientation=0x22, angles=np.linspace(-10, 10, A), scatterers=[(0.0, 0.0, 0.7 * z1)])
    if chirp:
        acq.filters = [cfg.matched_chirp_filter(FS / 2, L / (FS / 2), 2e6, 8e6)]
    else:
        acq.filters = [cfg.kaiser_filter(FS / 2, FD / 2, length=L)]
    return acq


KINDS = (DK.Int16, DK.Float16, DK.Float32)
DECIMATION_CASES = {}
for _i, (_D, _kind) in enumerate((d, k) for d in (2, 3, 4, 8) for k in KINDS):
    _L = (7, 36, 101)[_i % 3]
    _decode = _i % 2 == 1
    _A = (12, 16, 20)[(_i // 2) % 3]
    DECIMATION_CASES[f"D{_D}_{_kind.name}_L{_L}_A{_A}_{'decode' if _decode else 'das'}"] = (_D, _kind, _L, _A, _decode, False)
# D = 8 with 101 taps: lds_t = 16 x (8*64 + 100) x 8 B + 8 KiB > 64 KiB -- the 256-thread form in front of Decode
DECIMATION_CASES["D8_Int16_L101_A16_decode_untransposed"] = (8, DK.Int16, 101, 16, True, False)
DECIMATION_CASES["D2_Int16_chirp_A12_decode"] = (2, DK.Int16, 48, 12, True, True)
DECIMATION_CASES["D2_Float32_chirp_A20_das"] = (2, DK.Float32, 48, 20, False, True)


def ragged_case(S_, demod, seed):
    stages = (S.Demodulate, S.DAS) if demod else (S.Decode, S.DAS)
    fs_das = FS / 2 if demod else FS
    z1 = 0.8 * cfg.SPEED_OF_SOUND * (S_ / (2 if demod else 1) / fs_das) / 2
    return cfg.rca(f"ragged_{S_}_{'demod' if demod else 'decode'}", 8, 4, S_, (12, 1, 16), (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1),
                   seed=seed, stages=stages, decode=0 if demod else 1, fs=FS, fd=FD, pitch=PITCH,
                   angles=np.linspace(-5, 5, 4), scatterers=[(0.0, 0.0, 0.6 * z1)])


DECODE_KINDS = (DK.Int16, DK.Float16, DK.Float32Complex)


def decode_order_case(A, kind):
    S_ = 200 if A >= 40 else 1000
    Cn = 4
    z1 = 0.8 * cfg.SPEED_OF_SOUND * (S_ / FS) / 2
    return cfg.rca(f"decode_A{A}_{kind.name}", Cn, A, S_, (8, 1, 12), (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1), seed=500 + A,
                   data_kind=kind, stages=(S.Decode, S.DAS), decode=1, fs=FS, fd=FD, pitch=PITCH, angles=np.linspace(-5, 5, A))


# (a pipeline must start with Decode or Demodulate, lib .c:305-309, and Demodulate takes real RF only: {DAS} and {Filter, DAS}
# are written with a Decode that decode_mode None drops)
F16C_STAGES = {"das": (S.Decode, S.DAS), "decode": (S.Decode, S.DAS), "filter": (S.Decode, S.Filter, S.DAS)}


def float16_complex_case(pipeline):
    S_ = 512
    z1 = 0.8 * cfg.SPEED_OF_SOUND * (S_ / FS) / 2
    acq = cfg.rca(f"f16c_{pipeline}", 8, 4, S_, (12, 1, 16), (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1), seed=600 + len(pipeline),
                  data_kind=DK.Float16Complex, stages=F16C_STAGES[pipeline], decode=1 if pipeline == "decode" else 0,
                  fs=FS, fd=FD, pitch=PITCH, angles=np.linspace(-5, 5, 4))
    if pipeline == "filter":
        acq.filters = [cfg.matched_chirp_filter(FS, 2e-6, 2e6, 8e6)]
    return acq


D, I = P.DataKind, P.InterpolationMode
LO3, HI3 = (-2e-3, -2e-3, 3e-3), (2e-3, 2e-3, 9e-3)


def acquisitions():
    out = {}
    out["rca_i16"] = cfg.rca("rca_hilbert", 16, 3, 512, (16, 16, 1), (-2e-3, 0, 3e-3), (2e-3, 0, 9e-3), seed=71, demodulate=False)
    out["rca_f32_cubic_cw"] = cfg.rca("rca_hilbert_f32", 16, 4, 512, (12, 10, 3), LO3, HI3, seed=72, demodulate=False,
                                      data_kind=D.Float32, interp=I.Cubic, cw=True, orientation=0x12)
    out["hercules_decode"] = cfg.hercules("hercules_hilbert", 16, 8, 512, (8, 8, 6), LO3, HI3, seed=73, data_kind=D.Float16)
    out["forces_decode"] = cfg.forces("forces_hilbert", 16, 8, 512, (16, 1, 12), LO3, HI3, seed=74)
    for acq in out.values():
        with_hilbert(acq)
    return out


def with_hilbert(acq):
    """{Decode, DAS} -> {Decode, Hilbert, DAS}"""
    bp = acq.bp
    assert list(bp.compute_stages[:2]) == [int(S.Decode), int(S.DAS)]
    bp.compute_stages[1], bp.compute_stages[2] = int(S.Hilbert), int(S.DAS)
    bp.compute_stages_count = 3
    return acq


RAGGED_SAMPLES = (130, 1001)


def ragged_acquisition(samples):
    """ragged_case's decoded ragged rows with the stage behind the Decode: a wave's window is 64 + 62 samples, so 130
    leaves a last group of two outputs whose window ends 62 samples past the row, and 1001 an odd row"""
    acq = with_hilbert(ragged_case(samples, False, seed=800 + samples))
    acq.name = f"ragged_{samples}_hilbert"
    return acq


@pytest.fixture
def hilbert(bflib, oracle):
    assert bflib.library().beamformer_hip_enable_hilbert(1)
    oracle.enable_hilbert(True)
    yield
    bflib.library().beamformer_hip_enable_hilbert(0)
    oracle.enable_hilbert(False)


def nan_free(acq, das_in, label):
    """bar 1, with check_das_input's message"""
    nan = np.isnan(das_in)
    if nan.any():
        c, t, s = np.argwhere(nan)[0]
        raise AssertionError(f"{label}: {int(nan.sum())} DAS-input elements are NaN (read without having been written this frame), "
                             f"first at channel {c} transmit {t} sample {s} of {das_in.shape[2]} "
                             f"(decimation {acq.bp.decimation_rate}: samples [{das_in.shape[2] // max(1, acq.bp.decimation_rate)}, "
                             f"{das_in.shape[2]}) are the filter's tail)")


def first_difference(a, b):
    diff = as_bits(a) != as_bits(b)
    return f"{int(diff.sum())} scalars differ, first at {np.argwhere(diff)[0]} of {diff.shape}"


def push_burst(bflib, hooks, acq, rf, mode, poison=True):
    """(frames, [DAS input of frame k], route) of one burst of the RF frames `rf`"""
    L = bflib.library()
    if poison:
        hooks.set("SCRATCH_POISON")
    else:
        hooks.clear("SCRATCH_POISON")
    L.beamformer_hip_set_das_path(mode)
    try:
        frames = bflib.beamform_burst(acq.bp, rf, acq.filters).copy()
        route = bflib.last_burst_info().route
        inputs = [bflib.das_input(acq.bp, k) for k in range(len(rf))]
        newest = bflib.das_input(acq.bp)
        with pytest.raises(bflib.BeamformerError) as refused:
            bflib.das_input(acq.bp, len(rf))
    finally:
        L.beamformer_hip_set_das_path(0)
    assert refused.value.kind == P.LibError.InvalidAccess, "a frame index past the burst's frames is InvalidAccess"
    assert np.array_equal(as_bits(newest), as_bits(inputs[-1])), "beamformer_hip_copy_das_input after a burst: not the last frame's"
    return frames, inputs, route
