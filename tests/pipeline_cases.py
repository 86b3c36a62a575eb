"""The pre-DAS pipeline matrix: stage lists a client may push that the named cases (tests/cases.py) never plan -- two and three
filter stages, filter slots other than 0, Filter and Demodulate stages that store Int16 or binary16, stages that feed Decode or read
its layout, chains of up to six launches in front of DAS -- at the smallest shapes that still reach every launch form, and the host
audit every one of them has to pass before it may be launched: no stage writes past the inter-stage buffer the executor allocates.

Plain module (no tests): tests/test_pipelines_host.py checks it without a device, tests/test_gpu_pipelines.py runs it on one.

A pipeline is (data kind, stages, filter slot per stage, transmits A, decimation D, samples S, decode mode); `build` makes the
acquisition: 8 channels, a 12 x 1 x 16 grid, linear interpolation, no coherency weighting, seeded noise RF.  Int16 RF is divided by
8 so that no Int16-stored stage leaves the range in which host and device convert alike (the error model asserts the bound).
The four filter slots hold filters of distinct lengths and delays: a stage that reads the wrong slot cannot pass."""
import dataclasses

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P

S = P.ShaderKind
DK = P.DataKind
FS, FD, PITCH = 25e6, 6.25e6, 0.3e-3
CHANNELS, POINTS = 8, (12, 1, 16)
TRANSMITS, DECIMATIONS = (1, 2, 4, 12, 20), (1, 2, 3)
# compute_stage_parameters values: the C ABI keeps the low byte and the planner takes it modulo the slot count, so the highest value a
# client can write, 255, names slot 3
SLOT_VALUES = (0, 1, 3, 255)
KIND_BYTES = {0: 2, 1: 4, 2: 4, 3: 8, 4: 2, 5: 4}
PRE_DAS = (int(S.Reshape), int(S.Decode), int(S.Filter), int(S.Demodulate), int(S.Hilbert))


def filters():
    """slot 0: Kaiser low-pass, 36 taps; slot 1: complex matched chirp, 12 taps (sum of |taps| about 8: the bar of what follows a
    chirp grows by that factor); slot 2: Kaiser, 21 taps; slot 3: Kaiser, 7 taps"""
    return [cfg.kaiser_filter(FS / 2, FD / 2, length=36),
            cfg.matched_chirp_filter(FS / 2, 12.5 / (FS / 2), -2e6, 2e6),
            cfg.kaiser_filter(FS / 2, FD / 2, length=21, beta=4.0),
            cfg.kaiser_filter(FS / 2, FD / 2, length=7, beta=3.0)]


@dataclasses.dataclass(frozen=True)
class Pipeline:
    name: str
    kind: int
    stages: tuple            # as pushed, DAS last
    slots: tuple = ()        # compute_stage_parameters per pushed stage (missing: 0)
    A: int = 4
    D: int = 1
    S: int = 512
    decode: int = 1
    seed: int = 0


def build(p, swap=None):
    """the acquisition of pipeline `p`; swap = (slot a, slot b): the same with those two slots' filters exchanged"""
    demod = int(S.Demodulate) in [int(s) for s in p.stages]
    # the image ends at 0.7 of what a row records after decimation has left 1 / D of it (the filter's zero tail is
    # tests/test_gpu_stages.py's test_decimation's subject)
    z1 = 0.7 * cfg.SPEED_OF_SOUND * (p.S / FS) / 2 / (p.D if demod else 1)
    acq = cfg.rca(p.name, CHANNELS, p.A, p.S, POINTS, (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1), seed=9000 + p.seed, data_kind=DK(p.kind),
                  stages=tuple(S(int(s)) for s in p.stages), decimation=p.D, decode=p.decode, fs=FS, fd=FD, pitch=PITCH,
                  angles=np.linspace(-5, 5, p.A) if p.A > 1 else np.zeros(1))
    for i in range(len(p.stages)):
        acq.bp.compute_stage_parameters[i] = p.slots[i] if i < len(p.slots) else 0
    if P.DATA_KIND_NUMPY[int(p.kind)] == "int16":
        acq.rf = (acq.rf // 8).astype(np.int16)
    acq.filters = filters()
    if swap is not None:
        a, b = swap
        acq.filters[a], acq.filters[b] = acq.filters[b], acq.filters[a]
    return acq


# ------------------------------------------------------------------------------------------------ the curated list

def _p(name, kind, stages, slots=(), **kw):
    return Pipeline(name, int(kind), tuple(int(s) for s in stages) + (int(S.DAS),), tuple(slots), **kw)


Dc, F, Dm = S.Decode, S.Filter, S.Demodulate

CURATED = [
    # Demodulate / Filter that store Int16Complex (a stage between two don't-care neighbours keeps its input kind)
    _p("i16_demod_filter", DK.Int16, (Dm, F), (0, 1, 0)),
    _p("i16_demod_filter_D2", DK.Int16, (Dm, F), (0, 3, 0), D=2),
    _p("i16_demod_filter_D3_A12", DK.Int16, (Dm, F), (1, 0, 0), D=3, A=12),
    _p("i16_demod_filter_filter", DK.Int16, (Dm, F, F), (3, 0, 3, 0), A=2),
    _p("i16_demod_demod", DK.Int16, (Dm, Dm), (0, 3, 0)),
    # ... that feed Decode: Filter in the transposing form without demodulation, ragged blocks of 16 transmits
    _p("i16_demod_filter_decode", DK.Int16, (Dm, F, Dc), (3, 0, 0, 0)),
    _p("i16_demod_filter_decode_A20", DK.Int16, (Dm, F, Dc), (0, 255, 0, 0), A=20),
    _p("f32_demod_filter_decode_A20", DK.Float32, (Dm, F, Dc), (0, 1, 0, 0), A=20),
    _p("f16_demod_demod_decode_A12", DK.Float16, (Dm, Dm, Dc), (0, 3, 0, 0), A=12),
    _p("f32_demod_demod_decode_A20_D2", DK.Float32, (Dm, Dm, Dc), (3, 0, 0, 0), A=20, D=2),
    # the scratch overrun of the parent commit: Demodulate writes with the root's strides, counted in complex elements
    _p("f32_demod_filter", DK.Float32, (Dm, F), (0, 1, 0)),
    _p("f32_demod_filter_D2", DK.Float32, (Dm, F), (1, 0, 0), D=2),
    _p("f16_demod_filter_D3", DK.Float16, (Dm, F), (0, 3, 0), D=3),
    _p("f16_demod_filter_S1001", DK.Float16, (Dm, F), (0, 1, 0), S=1001),
    # Filter without demodulation on every kind that has no case yet (decode off: the Decode stage is dropped)
    _p("i16_filter", DK.Int16, (Dc, F), (0, 0, 0), decode=0),
    _p("i16c_filter", DK.Int16Complex, (Dc, F), (0, 1, 0), decode=0),
    _p("f32c_filter", DK.Float32Complex, (Dc, F), (0, 3, 0), decode=0),
    _p("f16_filter", DK.Float16, (Dc, F), (0, 0, 0), decode=0),
    # complex chirp taps on real samples: only the real parts enter
    _p("f32_filter_chirp", DK.Float32, (Dc, F), (0, 1, 0), decode=0),
    _p("i16_filter_chirp_filter", DK.Int16, (Dc, F, F), (0, 1, 3, 0), decode=0),
    # Decode whose output stays in decode layout, and stages that read it
    _p("f32_decode_demod", DK.Float32, (Dc, Dm), (0, 0, 0)),
    _p("f32_decode_filter_demod", DK.Float32, (Dc, F, Dm), (0, 3, 0, 0)),
    _p("f16_demod_decode_filter", DK.Float16, (Dm, Dc, F), (0, 0, 1, 0)),
    _p("i16c_decode_filter_filter", DK.Int16Complex, (Dc, F, F), (0, 0, 1, 0)),
    _p("f32c_decode_filter_decode", DK.Float32Complex, (Dc, F, Dc), (0, 3, 0, 0)),
    _p("f16c_decode_filter_filter_filter", DK.Float16Complex, (Dc, F, F, F), (0, 0, 3, 1, 0)),
    _p("f16_decode_filter_decode_filter", DK.Float16, (Dc, F, Dc, F), (0, 3, 0, 0, 0)),
    _p("i16_decode_filter_filter", DK.Int16, (Dc, F, F), (0, 3, 0, 0)),
    _p("i16_decode_decode", DK.Int16, (Dc, Dc), ()),
    _p("f32_decode_decode_A12", DK.Float32, (Dc, Dc), (), A=12),
    _p("f16c_decode_decode_filter_A2", DK.Float16Complex, (Dc, Dc, F), (0, 0, 3, 0), A=2),
    # real element kinds in front of Decode (never the transposing form), A = 20 and A = 1
    _p("f32_decode_filter_decode_A20", DK.Float32, (Dc, F, Dc), (0, 0, 0, 0), A=20),
    _p("i16_decode_filter_decode_A12", DK.Int16, (Dc, F, Dc), (0, 3, 0, 0), A=12),
    _p("f16_decode_filter_A1", DK.Float16, (Dc, F), (0, 3, 0), A=1),
    # long chains: the scratch ping-pong beyond two hops, up to six launches.  (A Filter that reads decode layout takes its windows
    # from the buffer's first few hundred elements -- the first samples of every row, filter.glsl ignores the sample stride -- so a
    # stage in front of it keeps a short filter, whose first outputs are not all warm-up, and few transmits.)
    _p("f32_decode_filter_decode_filter_filter", DK.Float32, (Dc, F, Dc, F, F), (0, 0, 0, 3, 1, 0)),
    _p("i16_demod_filter_decode_filter_decode", DK.Int16, (Dm, F, Dc, F, Dc), (3, 1, 0, 3, 0, 0), A=2),
    _p("f16_decode_filter_filter_decode_filter_S1001", DK.Float16, (Dc, F, F, Dc, F), (0, 3, 0, 0, 3, 0), S=1001),
    _p("i16c_decode_filter_decode_filter_filter", DK.Int16Complex, (Dc, F, Dc, F, F), (0, 3, 0, 3, 1, 0)),
    _p("f32c_decode_filter_filter_filter_filter", DK.Float32Complex, (Dc, F, F, F, F), (0, 0, 1, 3, 255, 0), A=2),
    _p("f32_demod_filter_demod_decode_filter", DK.Float32, (Dm, F, Dm, Dc, F), (0, 3, 0, 0, 3, 0)),
]
CURATED = [dataclasses.replace(p, seed=i) for i, p in enumerate(CURATED)]
BY_NAME = {p.name: p for p in CURATED}
assert len(BY_NAME) == len(CURATED)

# the chains of section "bursts", "order independence" and "frame graphs" of tests/test_gpu_pipelines.py
LONG_CHAINS = ["f32_decode_filter_decode_filter_filter", "i16_demod_filter_decode_filter_decode",
               "i16c_decode_filter_decode_filter_filter", "f32_demod_filter_demod_decode_filter"]


# ------------------------------------------------------------------------------------------------ random draws

RANDOM_SEEDS = range(96)
# how many stages follow the first: short chains more often -- every 16-bit hop and every Decode of A transmits (an orthogonal transform
# scaled by 1 / A: the signal falls by sqrt(A), its worst-case bound does not) costs signal against the bar, and a draw whose bar
# exceeds its signal checks nothing (`kept`)
FURTHER_STAGES = (0.4, 0.3, 0.2, 0.1)


def draw_pipeline(seed):
    """a client-valid stage list that ends in exactly one DAS: the data kind, Decode or Demodulate first (a complex kind starts with
    Decode and holds no Demodulate, lib .c:285-309), 1 to 4 further stages of {Decode, Filter, Demodulate}; a slot value per stage,
    the decode mode, the decimation and the transmit count"""
    rng = np.random.default_rng(77000 + seed)
    kind = int(rng.integers(0, 6))
    is_complex = P.DATA_KIND_COMPLEX[kind]
    pool = [int(Dc), int(F)] if is_complex else [int(Dc), int(F), int(Dm)]
    stages = [int(Dc) if is_complex else int(rng.choice([int(Dc), int(Dm)]))]
    stages += [int(rng.choice(pool)) for _ in range(int(rng.choice([1, 2, 3, 4], p=FURTHER_STAGES)))]
    stages.append(int(S.DAS))
    slots = tuple(int(rng.choice(SLOT_VALUES)) for _ in stages)
    decode = int(rng.integers(0, 2))
    D = int(rng.choice(DECIMATIONS))
    A = int(rng.choice(TRANSMITS))
    return Pipeline(f"draw{seed:02d}", kind, tuple(stages), slots, A=A, D=D, S=512, decode=decode, seed=100 + seed)


# A pipeline checks something only where its signal stands above its bar: of the DAS-input elements that can be nonzero (magnitude
# bound > 0: not a decimated row's tail) more than this share must have |oracle value| > bar.  Below it an all-zero DAS input, a wrong
# slot or a wrong stride would pass the element-wise check.
SIGNAL_SHARE = 0.5


def signal_share(bflib, oracle, acq, ref_in):
    """the share of the live DAS-input elements whose oracle value (the larger of |re|, |im|) exceeds the element's bar; 1.0 where
    every stage is exact (the check is bit-identity there)"""
    from tests import stage_checks as stages
    bflib.library().beamformer_reserve_parameter_blocks(1)
    exact, mag, bar = stages.stage_bounds(bflib, oracle, acq, stages.plan_of(bflib, acq))
    if exact:
        return 1.0
    value = np.maximum(np.abs(ref_in.real), np.abs(ref_in.imag)) if np.iscomplexobj(ref_in) else np.abs(ref_in)
    live = mag > 0
    return float(np.mean(value[live] > bar[live])) if live.any() else 0.0


def kept(bflib, oracle, p):
    """(acquisition, oracle frame, flags, oracle DAS input) when the draw is kept, else a reason: the oracle plans it, its frame is
    not empty, its DAS input is not all zero and stands above the bar on more than SIGNAL_SHARE of its live elements"""
    acq = build(p)
    if oracle.plan(acq.bp, acq.filters) is None:
        return "the oracle does not plan it"
    captured = {}
    ref, _ = oracle.beamform(acq.bp, acq.rf, acq.filters, das_input=captured)
    if not np.any(captured["data"]):
        return "the DAS input is all zero"
    ok = ~np.isnan(ref)
    if not ok.any() or not np.any(ref[ok]):
        return "the frame is empty"
    try:
        share = signal_share(bflib, oracle, acq, captured["data"])
    except AssertionError as refused:
        if "Int16 store of magnitudes" not in str(refused):
            raise
        return "an Int16-stored stage can leave the range in which host and device convert alike"
    if not share > SIGNAL_SHARE:
        return f"the bar exceeds the signal on {100 * (1 - share):.0f} % of the live DAS-input elements"
    return acq, ref, None, captured["data"]


# ------------------------------------------------------------------------------------------------ the extent audit

def write_extents(plan, bp):
    """[(stage index, stage kind, bytes)]: one past the last byte every stage in front of DAS writes into its inter-stage buffer --
    (sum_k out_stride[k] (n[k] - 1) + 1) elements of its output kind over n = (das_samples, channels, transmits); a filter that takes
    complex samples and stores real ones writes a second plane channels x das_samples x transmits scalars further on.  The same
    formula as csrc/planner.cpp sizes `intermediate_bytes` with and tests/plan_fuzz.cpp checks; restated here, not asked of the
    library."""
    n = (int(plan.das_samples), int(bp.channel_count), int(bp.acquisition_count))
    out = []
    for i in range(plan.stage_count):
        st = plan.stages[i]
        if int(st.kind) == int(S.DAS):
            break
        if int(st.kind) not in PRE_DAS:
            continue
        last = sum(int(st.out_stride[k]) * (n[k] - 1) for k in range(3))
        if int(st.kind) in (int(F), int(Dm)) and st.in_kind & 1 and not st.out_kind & 1:
            last += n[0] * n[1] * n[2]
        out.append((i, int(st.kind), (last + 1) * KIND_BYTES[int(st.out_kind)]))
    return out


def audit(plan, bp):
    """asserts that no stage in front of DAS writes past the buffer the executor allocates for the hop.  The allocated size is asked
    of the library: beamformer_hip_describe_plan reports the planner's `intermediate_bytes`, the very number commit_block hands to
    DeviceBuffer::ensure (+ 64 bytes) for both ping-pong buffers and that a burst takes as its frame stride (csrc/executor.cpp).
    The next stage may read `intermediate_bytes` bytes of it (in_elements), so everything written can be read."""
    allocated = int(plan.intermediate_bytes)
    extents = write_extents(plan, bp)
    for i, kind, extent in extents:
        assert extent <= allocated, (f"stage {i} ({S(kind).name}, out strides {list(plan.stages[i].out_stride)}, out kind "
                                     f"{DK(int(plan.stages[i].out_kind)).name}) writes up to byte {extent} of a buffer of {allocated} bytes")
    # reads: Reshape, Filter, Demodulate and Hilbert bound theirs (in_elements); Decode reads das_samples x channels x transmits
    # elements of its input kind unchecked, from the RF when it is the first launch
    rf_bytes = int(bp.channel_count) * int(bp.acquisition_count) * int(bp.sample_count) * KIND_BYTES[int(bp.data_kind)]
    for i, kind, _ in extents:
        if kind == int(Dc):
            reads = int(plan.das_samples) * int(bp.channel_count) * int(bp.acquisition_count) * KIND_BYTES[int(plan.stages[i].in_kind)]
            assert reads <= (allocated if i else rf_bytes), f"stage {i} (Decode) reads {reads} bytes of {allocated if i else rf_bytes}"
    return extents, allocated


# ------------------------------------------------------------------------------------------------ signatures

def layout(stride, plan, bp):
    Cn, A, Sn, Sd = int(bp.channel_count), int(bp.acquisition_count), int(bp.sample_count), int(plan.input_sample_count)
    stride = [int(v) for v in stride]
    if stride == [Cn * A, A, 1]:
        return "decode"
    if stride == [1, Sd * A, Sd]:
        return "das"
    if stride == [1, Sn * A, Sn]:
        return "root"
    return "other"


def signatures(oracle, acq):
    """the pre-DAS stages of the oracle's plan as (stage, in kind, out kind, in layout, out layout, taps): names, taps 'real' /
    'complex' for Filter and Demodulate and '' elsewhere; and the slot values the filter stages were pushed with"""
    plan = oracle.plan(acq.bp, acq.filters)
    assert plan is not None
    sigs, slots = [], []
    for i in range(plan.stage_count):
        st = plan.stages[i]
        if int(st.kind) == int(S.DAS):
            break
        taps = ""
        if int(st.kind) in (int(F), int(Dm)):
            fp = acq.filters[int(st.filter_slot) % P.FILTER_SLOTS]
            taps = "complex" if fp.complex and fp.kind == int(P.FilterKind.MatchedChirp) else "real"
            slots.append(int(st.filter_slot))
        sigs.append((S(int(st.kind)).name, DK(int(st.in_kind)).name, DK(int(st.out_kind)).name,
                     layout(st.in_stride, plan, acq.bp), layout(st.out_stride, plan, acq.bp), taps))
    return sigs, slots
