"""Dense stacks, sets of heads and ensembles on the GPU at the limits the headers promise (tests/dense_cases.py holds the cases
and says which code edge each is there for): every stack alone, every member of every set and every ensemble

  a. against the float64 restatement on the engine's own float32 embeddings - at ordinary scale within the project's 1e-4 gate,
     with every layer's largest |pre-activation| asserted inside 1..100; at 1e3 and 1e-6 within train_oracle.bound of the float32
     chain restatement (8 x that restatement's own deviation from float64);
  b. by bits - a member against its lone engine in both orders of the set, the one-kernel-per-op plan against the default plan,
     a window alone against itself inside 33 and 65, a call against its repetition, an ensemble against bd_ensemble_combine_host
     of the plain set's rows (tests/test_ensemble_gpu.py's rule);
  c. exactly - a softmax of length 1, rows that sum to 1, saturated sigmoid and tanh, finite everywhere;
  d. between guard words - the widest stack, the 64-member set and the 64-member ensemble, on poisoned workspaces;
  e. accepted - what bd_headset_members, bd_headset_outputs and bd_head_outputs report at each limit;
  f. the selects of dense_tile_walk - a hidden layer that overflows to +inf in some windows leaves the others alone.

Window counts are 1, 33 and 65; 1025 once, on the eight 2048-wide layers, in both plans.  References are computed once per case
from the 65 embedding rows of a headless engine (asserted to be the rows every engine returns) and shared."""
import numpy as np
import pytest

from tests import dense_cases as K
from tests import train_oracle

pytestmark = pytest.mark.gpu

HOP, STEP = K.HOP, 96
W_MAX = max(K.WINDOW_COUNTS)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Pool:
    """Engines by key, made on first use and closed with the module; rows and references, computed once."""

    def __init__(self):
        self.engines, self.rows_of, self.refs, self.lone_rows_of = {}, {}, {}, {}
        self.emb = None

    def engine(self, key, **kw):
        from buzzdetect_amd.engine import HipEngine
        if key not in self.engines:
            self.engines[key] = HipEngine(modelname=None, **kw)
        return self.engines[key]

    def drop(self, key):
        self.engines.pop(key).close()

    def embeddings(self):
        """The 65 embedding rows of an engine without a head: what every reference is computed from."""
        if self.emb is None:
            self.emb = self.engine("headless").embed(K.chunk(W_MAX), 0.96).numpy().copy()
            self.emb.setflags(write=False)
            assert self.emb.shape == (W_MAX, 1024) and self.emb.dtype == np.float32 and np.isfinite(self.emb).all()
        return self.emb

    def rows(self, key, windows, first=0):
        """(logits, embeddings) of engine `key` on `windows` windows from window `first`, both asked for in one call."""
        at = (key, windows, first)
        if at not in self.rows_of:
            logits, embs = self.engines[key].predict_batch([K.chunk(windows, first)], 0.96, want_embeddings=True)
            got = logits[0].numpy().copy(), embs[0].numpy().copy()
            assert got[0].shape == (windows, self.engines[key].n_classes) and got[0].dtype == np.float32
            # d. the caller's embeddings are a headless engine's
            assert same_bytes(got[1], self.embeddings()[first:first + windows]), f"{key}: embeddings differ from a headless engine's"
            for g in got:
                g.setflags(write=False)
            self.rows_of[at] = got
        return self.rows_of[at]

    def ref(self, name):
        """Case `name` on the 65 embedding rows: float64 output, per layer and row prefix the largest |pre-activation|, the
        float32 chain restatement."""
        if name not in self.refs:
            stack = K.stack_layers(name)
            taps = []
            f64 = K.stack_f64(self.embeddings(), stack, taps)
            maxima = [[float(np.abs(t[:w]).max()) for w in K.WINDOW_COUNTS] for t in taps]
            self.refs[name] = f64, maxima, K.stack_f32_chain(self.embeddings(), stack)
        return self.refs[name]

    def lone_rows(self, name, windows):
        """Rows of the engine that carries `name` alone (its engine is kept only while the case has a test of its own)."""
        if (name, windows) not in self.lone_rows_of:
            key = "lone:" + name
            keep = key in self.engines
            self.engine(key, head=K.head(name))
            for w in K.WINDOW_COUNTS:
                self.lone_rows_of[name, w] = self.rows(key, w)[0]
            if not keep:
                for w in K.WINDOW_COUNTS:
                    del self.rows_of[key, w, 0]
                self.drop(key)
        return self.lone_rows_of[name, windows]

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines = {}


@pytest.fixture(scope="module")
def pool():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    p = Pool()
    yield p
    p.close()


# ---------------------------------------------------------------------------------------------------- the checks
def check_member(pool, name, got, windows, first=0, what=""):
    """a. and c. for the columns `got` of case `name` on rows first .. first + windows of the 65."""
    c = K.STACKS[name]
    f64, maxima, chain = pool.ref(name)
    ref, chain = f64[first:first + windows], chain[first:first + windows]
    got = np.ascontiguousarray(got)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), f"{name}{what}: an output is not finite"
    delta = float(np.abs(got.astype(np.float64) - ref).max())
    bound, dev = train_oracle.bound(chain, ref)
    print(f"{name}{what} windows={windows}: max|delta|={delta:.3e} chain deviation={dev:.3e} "
          f"ratio={delta / dev if dev else float('nan'):.2f} bound={bound:.3e}")
    if K.is_scaled(name):
        assert delta <= bound, f"{name}{what}: {delta} beyond 8 x the float32 chain's own deviation {dev}"
    else:
        if first == 0:
            lo, hi = K.ORDINARY
            at = K.WINDOW_COUNTS.index(windows)
            assert all(lo <= layer[at] <= hi for layer in maxima), f"{name}: pre-activations {maxima} leave {lo}..{hi}"
        assert delta <= K.LOGIT_GATE, f"{name}{what}: {delta}"
    if c.acts[-1] == "softmax":
        if c.widths[-1] == 1:
            assert (got == 1.0).all(), f"{name}: a softmax of length 1 is 1.0"
        dsum = float(np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max())
        assert dsum <= 1e-5, f"{name}: softmax rows sum to 1 +- {dsum}"
    if c.acts[-1] in ("sigmoid", "tanh"):
        ref32 = ref.astype(np.float32)
        for end in (0.0, 1.0, -1.0):
            where = ref32 == end
            assert (got[where] == end).all(), f"{name}{what}: {int((got[where] != end).sum())} outputs saturated at {end} in " \
                                              f"float64 are not exactly {end}"


def check_engine(pool, key, columns, lone=()):
    """Engine `key` whose logits hold case columns[name] = slice: a. and c. for every member at 1, 33 and 65 windows, and b.:
    windows alone and inside a pass, the same call twice, the one-kernel-per-op plan; the members named in `lone` against
    their lone engines too."""
    eng = pool.engines[key]
    full = pool.rows(key, W_MAX)[0]
    for windows in K.WINDOW_COUNTS:
        got = pool.rows(key, windows)[0]
        assert same_bytes(got, full[:windows]), f"{key}: {windows} windows differ from themselves inside {W_MAX}"
        for name, cols in columns.items():
            check_member(pool, name, got[:, cols], windows, what=f" in {key}")
            if name in lone:
                assert same_bytes(got[:, cols], pool.lone_rows(name, windows)), f"{name} in {key} ({windows} windows) differs " \
                                                                                f"from its lone engine"
    for k in (32, 64):                                   # the last row of a tile, the lone row of the second workgroup
        alone = eng.predict(K.chunk(1, k), 0.96).numpy()
        assert same_bytes(alone[0], full[k]), f"{key}: window {k} alone differs from itself inside {W_MAX}"
    x = K.chunk(W_MAX)
    assert same_bytes(eng.predict(x, 0.96).numpy(), full), f"{key}: the same call twice"
    eng.set_fusion(stem=False, separable=False)
    try:
        per_op = eng.predict(x, 0.96).numpy().copy()                              # pooled rows in the workspace
        per_op_b, emb_b = eng.predict_batch([x], 0.96, want_embeddings=True)      # ... in the caller's embeddings
        per_op_b, emb_b = per_op_b[0].numpy(), emb_b[0].numpy()
    finally:
        eng.set_fusion()
    assert same_bytes(per_op, full), f"{key}: the one-kernel-per-op plan differs from the default plan (logits alone)"
    assert same_bytes(per_op_b, full) and same_bytes(emb_b, pool.embeddings()), f"{key}: ... (logits and embeddings)"


def columns_of(members):
    cols, at = {}, 0
    for m in members:
        n = K.STACKS[m].widths[-1]
        cols[m] = slice(at, at + n)
        at += n
    return cols


# ---------------------------------------------------------------------------------------------------- stacks alone
SHAPES = K.EDGES + sorted(set(K.FUSED.values())) + K.SOFTMAX + K.DEPTHS + K.WIDE + K.SCALED     # every distinct shape


@pytest.mark.parametrize("name", SHAPES)
def test_a_stack_alone(pool, name):
    """a. b. c. e. on an engine that carries the case alone: bd_head_attach's stack, or the fused head for one linear layer of
    at most 64 classes."""
    key = "lone:" + name
    eng = pool.engine(key, head=K.head(name))
    n = K.STACKS[name].widths[-1]
    assert eng.n_classes == n
    assert eng._lib.bd_head_outputs(eng._handle) == (0 if K.is_fused(name) else n)
    assert eng._lib.bd_headset_members(eng._handle) == 0
    check_engine(pool, key, {name: slice(0, n)})
    for w in K.WINDOW_COUNTS:
        pool.lone_rows_of[name, w] = pool.rows(key, w)[0]
    if name not in ("deep8_2048",):                      # (kept for the 1025-window test)
        pool.drop(key)


def test_1025_windows_through_eight_2048_wide_layers_in_both_plans(pool):
    """A full pass and a ragged pass of one window over the largest scratch the engine addresses: 2 x 2048 floats per window
    for 1024 windows, in the larger buffer (default plan) and behind the pooled rows of the smaller one (one kernel per op).
    float64 on rows 0, 1023 and 1024 only."""
    name = "deep8_2048"
    eng = pool.engine("lone:" + name, head=K.head(name))
    x = K.chunk(1025)
    logits, embs = eng.predict_batch([x], 0.96, want_embeddings=True)
    got, emb = logits[0].numpy().copy(), embs[0].numpy().copy()
    assert got.shape == (1025, 2048) and np.isfinite(got).all()
    assert same_bytes(got[:W_MAX], pool.lone_rows(name, W_MAX)) and same_bytes(emb[:W_MAX], pool.embeddings())
    rows = [0, 1023, 1024]
    taps = []
    ref = K.stack_f64(emb[rows], K.stack_layers(name), taps)
    maxima = [float(np.abs(t).max()) for t in taps]
    delta = float(np.abs(got[rows].astype(np.float64) - ref).max())
    dev = float(np.abs(K.stack_f32_chain(emb[rows], K.stack_layers(name)).astype(np.float64) - ref).max())
    print(f"{name} windows=1025 rows {rows}: max|delta|={delta:.3e} chain deviation={dev:.3e} ratio={delta / dev:.2f} "
          f"max|pre-activation| per layer {[round(m, 2) for m in maxima]}")
    assert all(K.ORDINARY[0] <= m <= K.ORDINARY[1] for m in maxima)
    assert delta <= K.LOGIT_GATE
    for k in (1023, 1024):
        assert same_bytes(eng.predict(K.chunk(1, k), 0.96).numpy()[0], got[k]), f"window {k} alone differs from itself inside 1025"
    eng.set_fusion(stem=False, separable=False)
    try:
        per_op = eng.predict(x, 0.96).numpy().copy()
        per_op_b, _ = eng.predict_batch([x], 0.96, want_embeddings=True)
        assert same_bytes(per_op, got) and same_bytes(per_op_b[0].numpy(), got)
    finally:
        eng.set_fusion()
    pool.drop("lone:" + name)


# ---------------------------------------------------------------------------------------------------- sets
def lone_partners(members):
    """The members held to their lone engines by bits: all of them - except in the two sets of 64 and 16 members of ONE shape,
    where the first twelve (every pair of activations the shape comes in) and the last (the last columns of the row) stand for
    the rest; an engine per member would make those two tests several seconds long.  Every member is still held to float64."""
    return set(members) if len({tuple(K.STACKS[m].widths) for m in members}) > 1 or len(members) <= 13 else \
        set(members[:12] + members[-1:])


@pytest.mark.parametrize("name", sorted(K.SETS))
def test_a_set(pool, name):
    """a. b. c. e. for every member of the set; where the table says so, in reverse order too (every member's columns move)."""
    s = K.SETS[name]
    orders = [("fwd", s.members)] + ([("rev", s.members[::-1])] if name in K.REVERSED else [])
    for tag, members in orders:
        key = f"set:{name}:{tag}"
        eng = pool.engine(key, heads={m: K.head(m) for m in members})
        lib = eng._lib
        # e. accepted at the limit, and reported
        assert lib.bd_headset_members(eng._handle) == len(members) and lib.bd_head_outputs(eng._handle) == 0
        assert lib.bd_headset_outputs(eng._handle) == K.set_outputs(members) == eng.n_classes
        if s.n_members is not None:
            assert lib.bd_headset_members(eng._handle) == 64
        if s.outputs is not None:
            assert lib.bd_headset_outputs(eng._handle) == 2048
        check_engine(pool, key, columns_of(members), lone=lone_partners(s.members))
        pool.drop(key)


# ---------------------------------------------------------------------------------------------------- ensembles
@pytest.mark.parametrize("name", sorted(K.ENSEMBLES))
def test_an_ensemble(pool, name):
    """The plain set of the ensemble's members (a. c. for every member) and the ensemble over it: every unit is
    bd_ensemble_combine_host of the plain set's rows - `mean` by bits, `mean_probability` within 8 x the float32 statement's
    error (tests/test_ensemble_gpu.py::check_unit) - and a pass-through keeps its member's bits."""
    from tests.test_ensemble_gpu import check_unit
    units = K.ENSEMBLES[name].units
    members = K.ensemble_members(name)
    plain_key = "plain:" + "+".join(u for u, _, _, _ in units) + ":" + members[0]
    if plain_key not in pool.engines:
        pool.engine(plain_key, heads={m: K.head(m) for m in members})
        check_engine(pool, plain_key, columns_of(members))
    key = "ens:" + name
    eng = pool.engine(key, heads=K.ensemble_heads(name))
    lib = eng._lib
    assert lib.bd_headset_members(eng._handle) == len(members) and lib.bd_headset_outputs(eng._handle) == K.set_outputs(members)
    assert lib.bd_ensemble_count(eng._handle) == len(units)
    assert lib.bd_ensemble_outputs(eng._handle) == eng.n_classes == sum(K.STACKS[n[0]].widths[-1] for _, n, _, _ in units)
    cols = columns_of(members)
    for windows in K.WINDOW_COUNTS:
        wide = pool.rows(plain_key, windows)[0]
        got = pool.rows(key, windows)[0]
        assert np.isfinite(got).all()
        assert same_bytes(got, pool.rows(key, W_MAX)[0][:windows])
        for (unit, names, combine, link), part in zip(units, eng.split(got).values()):
            member_rows = np.ascontiguousarray(wide[:, cols[names[0]].start:cols[names[-1]].stop])
            if combine is None:
                assert same_bytes(part, member_rows), f"{name}/{unit}: a pass-through changed its member's bits"
            else:
                check_unit(np.ascontiguousarray(part), member_rows, len(names), combine, link, f"{name}/{unit} ({windows} windows)")
    full = pool.rows(key, W_MAX)[0]
    x = K.chunk(W_MAX)
    assert same_bytes(eng.predict(x, 0.96).numpy(), full)
    for k in (32, 64):
        assert same_bytes(eng.predict(K.chunk(1, k), 0.96).numpy()[0], full[k])
    eng.set_fusion(stem=False, separable=False)
    try:
        per_op_b, emb_b = eng.predict_batch([x], 0.96, want_embeddings=True)
        assert same_bytes(eng.predict(x, 0.96).numpy(), full) and same_bytes(per_op_b[0].numpy(), full)
        assert same_bytes(emb_b[0].numpy(), pool.embeddings())
    finally:
        eng.set_fusion()
    pool.drop(key)


# ---------------------------------------------------------------------------------------------------- hygiene
def hygiene_engines():
    return {
        "deep8_2048": lambda: dict(head=K.head("deep8_2048")),                                  # the widest stack
        "deep8_mixed": lambda: dict(head=K.head("deep8_mixed")),                                # K = 1, 3, 33, 65, 2047 in scratch
        "full64": lambda: dict(heads={m: K.head(m) for m in K.SETS["full64"].members}),         # the 64-member set
        "k64_softmax": lambda: dict(heads=K.ensemble_heads("k64_softmax")),                     # the k = 64 ensemble
    }


@pytest.mark.parametrize("which", sorted(hygiene_engines()))
def test_between_guard_words_on_poisoned_workspaces(pool, which):
    """d. Logits and embeddings between guard words, the workspace exactly as large as the library asks for and prefilled with
    zeros, NaNs and huge values in turn: nothing outside the rows changes, every element inside is written, the three patterns
    give the same bits (a never-written scratch column that reached an accumulator would carry its NaN into the row), and the
    embeddings are a headless engine's."""
    import torch
    from tests.gpu_guards import GuardedEngine
    from tests.test_hotpath_hygiene_gpu import guarded_run
    eng = GuardedEngine(modelname=None, **hygiene_engines()[which]())
    try:
        eng.exact = False
        want = eng.predict(K.chunk(33), 0.96).numpy().copy()
        eng.exact = True
        x = torch.from_numpy(K.chunk(33)).to(eng.device)
        for fused in (True, False):
            eng.set_fusion(stem=fused, separable=fused)
            for want_embeddings in (False, True):
                emb, logits = guarded_run(eng, [x], HOP, STEP, None, want_embeddings)
                assert same_bytes(logits, want) and np.isfinite(logits).all()
                if want_embeddings:
                    assert same_bytes(emb, pool.embeddings()[:33])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------- the selects of dense_tile_walk
def test_windows_whose_hidden_layer_overflows_leave_the_other_windows_alone(pool):
    """The 16-byte loads of dense_tile_walk reach round_up(K, 32) columns of a scratch row; what lies behind column K is
    replaced by zero, not multiplied by the zero-padded weights - the difference shows only when that word is not finite.
    This stack puts +inf there: layer 0 (relu) is zero for every window whose embedding feature k lies below a threshold and
    about 1e28 above it, layer 1 (linear, 2048 wide, weights 1e30) turns that into +inf in all 2048 columns of scratch region 1
    for windows 0 and 1 and leaves the bias for the windows below the threshold.  Layer 3 lands in region 1 again, rows 64 floats
    apart, 33 wide: columns 33..63 of row r still hold layer 1's row r // 32.  Layer 4 (K = 33) loads them.  The windows below
    the threshold must come out finite and within 8 x the float32 chain's own deviation from float64, in both plans."""
    from buzzdetect_amd import modeldir, weights as W
    emb = pool.embeddings()
    least = np.minimum(emb[0], emb[1])
    low_a, low_b = (emb[2:32] <= 0.85 * least).sum(axis=0), (emb[32:64] <= 0.85 * least).sum(axis=0)
    k = int((np.minimum(low_a, low_b) * (least > 0.05)).argmax())
    t = np.float32(0.925) * least[k]
    clean = np.flatnonzero(emb[:64, k] <= 0.85 * least[k])
    assert least[k] > 0.05 and (clean < 32).sum() >= 4 and (clean >= 32).sum() >= 4, "no feature separates windows 0 and 1 from the rest"
    s = np.float32(1e30)
    k0 = np.zeros((1024, 32), np.float32)
    k0[k] = s
    b0 = np.full(32, -s * t, np.float32)
    k1 = np.full((32, 2048), s, np.float32)
    rest = modeldir.glorot_layers([40, 33, 5], ["tanh", "relu", "linear"], seed=77, n_in=2048, gain=1.0)
    b1 = modeldir.glorot_layers([2048], ["linear"], seed=78, n_in=32)[0][1]
    stack = [(k0, b0, "relu"), (k1, b1, "linear")] + rest
    with np.errstate(over="ignore", invalid="ignore"):
        hidden = K.stack_f32_chain(emb, stack[:2])
    assert np.isposinf(hidden[:2]).all() and np.array_equal(hidden[clean], np.broadcast_to(b1, (len(clean), 2048)))
    ref = K.stack_f64(emb[clean], stack)
    bound, dev = train_oracle.bound(K.stack_f32_chain(emb[clean], stack), ref)
    eng = pool.engine("overflow", head=W.HeadWeights(stack, [f"c{i}" for i in range(5)]))
    try:
        for fused in (True, False):
            eng.set_fusion(stem=fused, separable=fused)
            got = eng.predict(K.chunk(W_MAX), 0.96).numpy()
            assert got.shape == (W_MAX, 5)
            assert np.isfinite(got[clean]).all(), "a window below the threshold picked up another window's +inf"
            delta = float(np.abs(got[clean].astype(np.float64) - ref).max())
            print(f"overflow stack ({'default' if fused else 'one kernel per op'} plan), feature {k}, {len(clean)} windows below the "
                  f"threshold: max|delta|={delta:.3e} chain deviation={dev:.3e} bound={bound:.3e}")
            assert delta <= bound
    finally:
        eng.set_fusion()
        pool.drop("overflow")
