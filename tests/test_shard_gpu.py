"""The sharded block exchange on the device (omm_amd/csrc/tail_kernels.hip: shard_interleave, owner_of_position, shard_pack_meta / shard_unpack_meta,
shard_masked_sizes / shard_take_offsets, shard_gather_contribution, shard_scatter_contributions, shard_codec_count / _write / _finish, codec_rank,
shard_scatter_streams; the host code of omm_host.cpp that drives them) at its ownership, layout and codec edges, through the C ABI: the four-phase API
(ommxShardedBegin ... Finish) with every rank in this process, the one-call bake (ommxShardedBakeRccl over ommxCommFromCollectives) with callbacks
written here that record what crosses the wire -- one rank without threads, several ranks as Python threads with a barrier that times out --, and the
multi-device ommCpuBake.  Every result is compared with the oracle's, every intermediate with the restatement of tests/shard_cases.py, byte for byte.
tests/test_shard_reference.py proves without a GPU what the cases cover."""
import ctypes as C
import threading
import traceback
import numpy as np
import pytest
import ommtest as ot
import tail_cases as tc
import shard_cases as sc

pytestmark = pytest.mark.gpu

BARRIER_SECONDS = 20.0
JOIN_SECONDS = 90.0
ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class Collectives(C.Structure):
    _fields_ = [("allReduceU32", ALLREDUCE), ("allGatherBytes", ALLGATHER), ("user", C.c_void_p)]


@pytest.fixture(scope="module")
def hip():
    h = ot.Hip()
    h.rt.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return h


@pytest.fixture(scope="module")
def dll(product):
    import omm_amd.sharded as sh
    d = sh.bind(product.dll)
    d.ommxCommFromCollectives.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    d.ommxRcclCommDestroy.argtypes = [C.c_void_p]
    d.ommxShardedBakeRccl.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    d.ommxGetDeviceBakeResultDesc.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ot.BakeResultDesc))]
    d.ommxDestroyDeviceBakeResult.argtypes = [C.c_void_p]
    return d


def timings(product, baker):
    import bench
    return bench.get_timings(product, baker)


class Baked:
    """a baker of the HIP library with the case's texture, its desc with the bulk arrays in device memory"""

    def __init__(self, product, hip, case, knobs=()):
        self.product, self.hip = product, hip
        self.baker = product.create_baker()
        for k, v in knobs:
            product.set_knob(self.baker, k, v)
        self.tex = product.create_texture(self.baker, [case["tex"]], alpha_cutoff=0.5)
        self.host_desc = ot.make_desc(self.tex, case["uv"], case["ix"], case["gmax"], **tc.desc_kw(case))
        self.bufs = [hip.upload(case["uv"]), hip.upload(case["ix"].astype(np.int32))]
        self.desc = ot.BakeInputDesc.from_buffer_copy(self.host_desc)
        self.desc.texCoords, self.desc.indexBuffer = self.bufs[0], self.bufs[1]
        if case["levels"] is not None:
            self.bufs.append(hip.upload(case["levels"]))
            self.desc.subdivisionLevels = self.bufs[2]

    def close(self):
        for p in self.bufs:
            self.hip.free(p)
        self.product.destroy_texture(self.baker, self.tex)
        self.product.destroy_baker(self.baker)


def four_phase(product, hip, dll, case, world, knobs=(), fill=0xCD):
    """every rank of a four-phase bake in this process; the two collectives on the host.  The gathered buffer holds rank r's bytes [0, contributionBytes[r])
    and `fill` everywhere else.  -> words of every rank before the sum, their sum, contributionBytes, strideBytes, contributions, results, activeItems"""
    B = Baked(product, hip, case, knobs)
    try:
        handles, words = [], []
        for r in range(world):
            h = C.c_void_p()
            assert dll.ommxShardedBegin(B.baker, C.byref(B.desc), r, world, C.byref(h)) == ot.SUCCESS
            handles.append(h)
        ptrs = []
        for h in handles:
            w, n = C.c_void_p(), C.c_uint64()
            assert dll.ommxShardedGetMeta(h, C.byref(w), C.byref(n)) == ot.SUCCESS
            assert n.value % 4 == 0
            ptrs.append((w, n.value))
            words.append(hip.download(w, 4 * n.value, np.uint32).reshape(4, -1).copy())
        assert len({n for _, n in ptrs}) == 1
        total = np.zeros_like(words[0])
        for w in words:
            total = total + w
        if total.size:
            for w, n in ptrs:
                hip.copy_htod(w, total.reshape(-1))
        contribs, nbytes, strides = [], [], []
        for h in handles:
            c, nb, st = C.c_void_p(), C.c_uint64(), C.c_uint64()
            assert dll.ommxShardedTail(h, C.byref(c), C.byref(nb), C.byref(st)) == ot.SUCCESS
            assert nb.value <= st.value
            contribs.append(hip.download(c, nb.value).copy())
            nbytes.append(nb.value)
            strides.append(st.value)
        assert len(set(strides)) == 1, strides
        stride = strides[0]
        host = np.full(stride * world, fill, np.uint8)
        for r, c in enumerate(contribs):
            host[r * stride:r * stride + len(c)] = c
        gathered = hip.upload(host)
        results = []
        for h in handles:
            out = C.c_void_p()
            assert dll.ommxShardedFinish(h, gathered, C.byref(out)) == ot.SUCCESS
            results.append(ot.device_result_to_host(product, hip, out))
        tm = timings(product, B.baker)
        for h in handles:
            assert dll.ommxShardedDestroy(h) == ot.SUCCESS
        hip.free(gathered)
        return dict(words=words, total=total, nbytes=nbytes, stride=stride, contribs=contribs, results=results, active=int(tm.activeItems))
    finally:
        B.close()


class Wire:
    """the transport of a one-call bake between the ranks of this process: a barrier with a time limit, one slot per rank for its send pointer, and the record
    of every all-gather: (bytesPerRank, host copy of `send`) per rank"""

    def __init__(self, hip, size):
        self.hip, self.size = hip, size
        self.barrier = threading.Barrier(size)
        self.slot = [None] * size
        self.sends = [[] for _ in range(size)]

    def wait(self):
        if self.size > 1:
            self.barrier.wait(timeout=BARRIER_SECONDS)           # (raises when a rank is missing: the callback then answers non-zero)

    def callbacks(self, rank):
        hip, rt = self.hip, self.hip.rt

        def all_reduce(_user, send, recv, count, op, stream):
            try:
                if rt.hipStreamSynchronize(stream) != 0:
                    return 1
                self.slot[rank] = send
                self.wait()
                acc = None
                for q in range(self.size):
                    part = hip.download(self.slot[q], 4 * count, np.uint32)
                    acc = part.copy() if acc is None else (acc + part if op == 0 else (np.maximum(acc, part) if op == 1 else np.minimum(acc, part)))
                self.wait()                                       # everybody has read every `send` (recv may be the same buffer)
                hip.copy_htod(recv, acc)
                return 0
            except Exception:                                     # (an exception must not unwind through the C frames)
                traceback.print_exc()
                return 1

        def all_gather(_user, send, recv, nbytes, stream):
            try:
                if rt.hipStreamSynchronize(stream) != 0:
                    return 1
                self.sends[rank].append((int(nbytes), hip.download(send, nbytes).copy()))
                self.slot[rank] = send
                self.wait()
                for q in range(self.size):
                    if rt.hipMemcpyAsync((recv or 0) + q * nbytes, self.slot[q], nbytes, 3, stream) != 0:
                        return 2
                if rt.hipStreamSynchronize(stream) != 0:
                    return 3
                self.wait()                                       # nobody reuses its `send` before all copies are done
                return 0
            except Exception:
                traceback.print_exc()
                return 1

        return ALLREDUCE(all_reduce), ALLGATHER(all_gather)


def one_call(product, hip, dll, case, world, knobs=()):
    """ommxShardedBakeRccl over callbacks of this file: one baker and one communicator per rank, ranks > 1 as threads.  -> results, recorded sends,
    timings of every rank"""
    wire = Wire(hip, world)
    codes, results, tms, errors = [None] * world, [None] * world, [None] * world, []

    def rank_body(r):
        try:
            B = Baked(product, hip, case, knobs)
            try:
                ar, ag = wire.callbacks(r)
                table = Collectives(ar, ag, None)
                comm = C.c_void_p()
                assert dll.ommxCommFromCollectives(C.byref(table), r, world, C.byref(comm)) == ot.SUCCESS
                out = C.c_void_p()
                codes[r] = dll.ommxShardedBakeRccl(B.baker, C.byref(B.desc), comm, C.byref(out))
                if codes[r] == ot.SUCCESS:
                    results[r] = ot.device_result_to_host(product, hip, out)
                    tms[r] = timings(product, B.baker)
                assert dll.ommxRcclCommDestroy(comm) == ot.SUCCESS
            finally:
                B.close()
        except Exception:
            errors.append((r, traceback.format_exc()))
            wire.barrier.abort()                                   # a rank that has failed must not leave the others waiting

    if world == 1:
        rank_body(0)
    else:
        threads = [threading.Thread(target=rank_body, args=(r,), daemon=True) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_SECONDS)
        assert not any(t.is_alive() for t in threads), "a rank thread is still running"
    assert not errors, errors
    assert codes == [ot.SUCCESS] * world, codes
    return dict(results=results, sends=wire.sends, timings=tms)


def all_equal(results, ref, name):
    for r, res in enumerate(results):
        assert res.same_as(ref), "%s rank %d/%d: %s" % (name, r, len(results), res.diff(ref))


def contributions_hold(run, ref, owners, world, name):
    con, nbytes, stride = sc.restate_contributions(ref, owners, world)
    assert run["nbytes"] == nbytes and run["stride"] == stride, (name, run["nbytes"], nbytes, run["stride"], stride)
    for r in range(world):
        assert np.array_equal(run["contribs"][r], con[r]), (name, r, np.nonzero(run["contribs"][r] != con[r])[0][:8])
    return con, nbytes, stride


# ---- O: ownership and interleave ----
_WORLD1_WORDS = {}


@pytest.mark.parametrize("world", sc.WORLDS)
@pytest.mark.parametrize("kind", sc.O_KINDS)
def test_ownership_and_interleave(product, hip, dll, kind, world):
    case = sc.o_case(kind, world)
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, world)
    n = len(inp["level"])
    run = four_phase(product, hip, dll, case, world)
    assert run["total"].shape[1] == n == run["active"]                                   # Nearest: every valid item is on the active list
    lst, pos_owner, counts = sc.list_items(inp["level"], world)
    for r in range(world):
        assert np.array_equal(run["words"][r][0] != 0, pos_owner == r), (case["name"], r)       # the mask of a classified item is never 0
        assert not run["words"][r][:, pos_owner != r].any()
    # the summed words at list position j are the one-rank words at natural position restate_interleave(cnt)[j]
    if case["name"] not in _WORLD1_WORDS:
        _WORLD1_WORDS[case["name"]] = run["total"] if world == 1 else four_phase(product, hip, dll, case, 1)["total"]
    w1 = _WORLD1_WORDS[case["name"]]
    a, perm = 0, []
    for cnt in counts:
        perm.append(a + sc.restate_interleave(int(cnt), world))
        a += cnt
    perm = np.concatenate(perm)
    assert np.array_equal(run["total"], w1[:, perm]), case["name"]
    # ... and both are the restated items': state masks, and the digest of the states the oracle decoded
    natural, _ = sc.natural_items(inp["level"])
    assert np.array_equal(w1[0], sc.item_masks(inp)[natural])
    dg = w1[2].astype(np.uint64) | (w1[3].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(dg, sc.item_digests(inp)[natural])
    assert np.array_equal(lst, natural[perm])
    contributions_hold(run, ref, own, world, case["name"])
    all_equal(run["results"], ref, case["name"])


def test_rank_and_world_size_out_of_range(product, hip, dll):
    case = sc.e_case("one-block")
    B = Baked(product, hip, case)
    try:
        for rank, world in ((0, 17), (2, 2), (16, 16), (0, 0)):
            h = C.c_void_p()
            assert dll.ommxShardedBegin(B.baker, C.byref(B.desc), rank, world, C.byref(h)) == ot.INVALID_ARGUMENT and not h.value
    finally:
        B.close()


# ---- E: empty exchanges ----
@pytest.mark.parametrize("kind", sc.E_KINDS)
def test_empty_exchanges(product, hip, dll, kind):
    case = sc.e_case(kind)
    ref, raw, _ = sc.reference(case)
    for world in (1, 2, 8):
        run = four_phase(product, hip, dll, case, world)
        if kind == "nothing-valid":
            assert run["total"].size == 0 and run["active"] == 0 and run["nbytes"] == [0] * world and run["stride"] == 256
        elif kind == "all-uniform":
            assert run["total"].shape[1] == len(case["uv"]) // 3 and run["nbytes"] == [0] * world and run["stride"] == 256
        else:
            own, rs, inp = sc.block_owners(case, raw, world)
            contributions_hold(run, ref, own, world, case["name"])
            assert sorted(run["nbytes"]) == [0] * (world - 1) + [16] and run["stride"] == 256
        all_equal(run["results"], ref, case["name"])
    one = one_call(product, hip, dll, case, 1)
    all_equal(one["results"], ref, case["name"] + " one call")
    if kind == "nothing-valid" or kind == "all-uniform":
        assert one["sends"] == [[]]                                                     # no OMM: nothing crosses


# ---- L: layout and raw scatter ----
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fmt", tc.FORMATS)
@pytest.mark.parametrize("kind", sc.L_KINDS)
def test_layout_and_padding(product, hip, dll, kind, fmt, world):
    case = sc.l_case(kind, fmt)
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, world)
    run = four_phase(product, hip, dll, case, world)                                      # (padding of the gathered buffer: 0xCD)
    assert run["active"] == len(inp["level"])
    contributions_hold(run, ref, own, world, case["name"])
    all_equal(run["results"], ref, case["name"])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_scatter_in_chunks_that_cut_blocks(product, hip, dll, fmt, world):
    case = sc.l_case("few", fmt)
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, world)
    _, nbytes, stride = sc.restate_contributions(ref, own, world)
    for knob in (256, 4352, sc.pad256(stride // 8)):
        assert knob != sc.pad256(stride // 8) or len(sc.chunk_sizes(stride, knob)) == 8
        run = four_phase(product, hip, dll, case, world, knobs=((ot.KNOB_SHARD_CHUNK_BYTES, knob),))
        contributions_hold(run, ref, own, world, case["name"])
        all_equal(run["results"], ref, "%s knob %d" % (case["name"], knob))


@pytest.mark.parametrize("world", [2, 3])
def test_duplicate_blocks_stay_with_the_lowest_work_item(product, hip, dll, world):
    case = sc.l_duplicates_case()
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, world)
    run = four_phase(product, hip, dll, case, world)
    assert run["active"] == len(inp["level"])
    contributions_hold(run, ref, own, world, case["name"])
    assert sum(run["nbytes"]) == ref.array_data.size
    all_equal(run["results"], ref, case["name"])


# ---- U: uniform blocks that every rank writes itself ----
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fmt,le,gt", [(f, le, gt) for f in tc.FORMATS for le, gt in sc.U_STATES[f]])
def test_uniform_blocks_are_synthesised_locally(product, hip, dll, fmt, le, gt, world):
    case = sc.u_case(fmt, le, gt)
    ref, raw, _ = sc.reference(case)
    for knobs in ((), ((ot.KNOB_SHARD_CHUNK_BYTES, 256),)):
        run = four_phase(product, hip, dll, case, world, knobs=knobs)
        assert run["active"] < len(ref.descs), (run["active"], len(ref.descs))           # settled uniform items never became active
        assert sum(run["nbytes"]) < ref.array_data.size
        assert not knobs or len(sc.chunk_sizes(run["stride"], 256)) > 1                   # several chunks: uniform blocks come with the first only
        all_equal(run["results"], ref, "%s knobs %r" % (case["name"], knobs))
    one = one_call(product, hip, dll, case, world)
    all_equal(one["results"], ref, case["name"] + " one call")


# ---- C: the device codec, observed on the wire ----
def exact_stream(product, hip, dll, case, knobs=()):
    ref, raw, _ = sc.reference(case)
    one = one_call(product, hip, dll, case, 1, knobs)
    all_equal(one["results"], ref, case["name"])
    want = sc.codec_encode(ref.array_data)
    tm = one["timings"][0]
    return ref, one, want, tm


def stream_holds(send, want, nbytes, name):
    n, got = send
    assert n == len(want) == len(got), (name, n, len(want))
    m = sc.stream_defined(nbytes, len(want))
    bad = np.nonzero((got != want) & m)[0]
    assert bad.size == 0, (name, "stream differs in %d bytes, first at %d" % (bad.size, bad[0]))
    assert np.array_equal(sc.codec_decode(got), sc.codec_decode(want))


@pytest.mark.parametrize("n", sc.C_SIZES)
def test_stream_of_a_whole_array(product, hip, dll, n):
    for fmt, le, gt in ((ot.FMT_4STATE, ot.T, ot.O), (ot.FMT_4STATE, ot.UT, ot.UO), (ot.FMT_2STATE, ot.T, ot.O)):
        case = sc.c_size_case(n, fmt, le, gt)
        ref, one, want, tm = exact_stream(product, hip, dll, case)
        assert len(one["sends"][0]) == 1
        stream_holds(one["sends"][0][0], want, ref.array_data.size, case["name"])
        assert tm.exchangeBytes == len(want) and tm.contributionBytes == ref.array_data.size


def test_stream_of_planned_raw_units(product, hip, dll):
    case = sc.c_pattern_case()
    ref, one, want, tm = exact_stream(product, hip, dll, case)
    sc.pattern_holds(case, ref.array_data)
    stream_holds(one["sends"][0][0], want, ref.array_data.size, case["name"])
    assert tm.exchangeBytes == len(want) and tm.contributionBytes == ref.array_data.size


def test_stream_of_ragged_totals(product, hip, dll):
    case = sc.ragged_case()
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, 1)
    con, nbytes, stride = sc.restate_contributions(ref, own, 1)
    one = one_call(product, hip, dll, case, 1)
    all_equal(one["results"], ref, case["name"])
    n, got = one["sends"][0][0]
    assert np.array_equal(sc.codec_decode(got)[:nbytes[0]], con[0]) and one["timings"][0].contributionBytes == stride


def test_stream_at_the_cap(product, hip, dll):
    case = sc.c_limit_case(0)
    ref, one, want, tm = exact_stream(product, hip, dll, case)
    assert len(want) == sc.comp_cap(ref.array_data.size)
    assert len(one["sends"][0]) == 1
    stream_holds(one["sends"][0][0], want, ref.array_data.size, case["name"])
    assert tm.exchangeBytes == len(want)


@pytest.mark.parametrize("knob", [256, 0])
def test_stream_one_unit_over_the_cap_goes_raw(product, hip, dll, knob):
    case = sc.c_limit_case(1)
    ref, one, want, tm = exact_stream(product, hip, dll, case, knobs=((ot.KNOB_SHARD_CHUNK_BYTES, knob),) if knob else ())
    stride = ref.array_data.size
    assert len(want) == sc.comp_cap(stride) + 16
    sends = one["sends"][0]
    assert [n for n, _ in sends] == sc.chunk_sizes(stride, knob), ([n for n, _ in sends], sc.chunk_sizes(stride, knob))
    assert np.array_equal(np.concatenate([b for _, b in sends]), ref.array_data)          # raw chunks of the contribution
    assert tm.exchangeBytes == stride == tm.contributionBytes


# ---- M: several ranks in one process (Python threads) ----
def streams_hold(one, ref, owners, world, name):
    con, nbytes, stride = sc.restate_contributions(ref, owners, world)
    want = [sc.codec_encode(sc.padded(c, stride)) for c in con]
    pitch = max(len(w) for w in want)
    for r in range(world):
        assert len(one["sends"][r]) == 1, (name, r, len(one["sends"][r]))
        n, got = one["sends"][r][0]
        assert n == pitch, (name, r, n, pitch)                                            # the pitch is the longest stream
        stream_holds((len(want[r]), got[:len(want[r])]), want[r], stride, "%s rank %d" % (name, r))
        assert np.array_equal(sc.codec_decode(got[:len(want[r])])[:nbytes[r]], con[r])
        assert one["timings"][r].exchangeBytes == pitch and one["timings"][r].contributionBytes == stride
    return want


def raw_chunks_hold(one, ref, owners, world, knob, name):
    """every rank sent raw chunks of its padded contribution, cut as shard_chunk_bytes says"""
    con, nbytes, stride = sc.restate_contributions(ref, owners, world)
    for r in range(world):
        assert [n for n, _ in one["sends"][r]] == sc.chunk_sizes(stride, knob), (name, r, [n for n, _ in one["sends"][r]])
        assert np.array_equal(np.concatenate([b for _, b in one["sends"][r]]), sc.padded(con[r], stride)), (name, r)
        assert one["timings"][r].exchangeBytes == stride == one["timings"][r].contributionBytes


def exchange_holds(one, ref, owners, world, name, knob=0):
    """streams if every rank's restated stream fits the restated cap, raw chunks from every rank if one does not"""
    con, nbytes, stride = sc.restate_contributions(ref, owners, world)
    longest = max(len(sc.codec_encode(sc.padded(c, stride))) for c in con)
    if longest <= sc.comp_cap(stride):
        streams_hold(one, ref, owners, world, name)
    else:
        raw_chunks_hold(one, ref, owners, world, knob, name)
    return longest <= sc.comp_cap(stride)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_as_threads_streams_of_different_lengths(product, hip, dll, world):
    case = sc.lengths_case(world)
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, world)
    one = one_call(product, hip, dll, case, world)
    all_equal(one["results"], ref, case["name"])
    want = streams_hold(one, ref, own, world, case["name"])
    assert len({len(w) for w in want}) >= 2


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_as_threads_empty_contributions(product, hip, dll, world):
    for case in (sc.o_case("tiny", world), sc.l_case("few", ot.FMT_4STATE)):
        ref, raw, _ = sc.reference(case)
        own, rs, inp = sc.block_owners(case, raw, world)
        con, nbytes, stride = sc.restate_contributions(ref, own, world)
        assert 0 in nbytes or world == 2, (case["name"], nbytes)
        one = one_call(product, hip, dll, case, world)
        all_equal(one["results"], ref, case["name"])
        compressed = exchange_holds(one, ref, own, world, case["name"])
        assert compressed == case["name"].startswith("O-tiny")                            # (the noise of L does not shrink: raw, empty ranks included)
    for kind in sc.E_KINDS:
        case = sc.e_case(kind)
        one = one_call(product, hip, dll, case, world)
        all_equal(one["results"], sc.reference(case)[0], case["name"])


def test_ranks_as_threads_uniform_blocks_at_world_8(product, hip, dll):
    """(worlds 2 and 3: test_uniform_blocks_are_synthesised_locally)"""
    for fmt in tc.FORMATS:
        for le, gt in sc.U_STATES[fmt]:
            case = sc.u_case(fmt, le, gt)
            one = one_call(product, hip, dll, case, 8)
            all_equal(one["results"], sc.reference(case)[0], case["name"])


@pytest.mark.parametrize("knob", [0, 4352])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_as_threads_one_rank_incompressible(product, hip, dll, world, knob):
    case = sc.mixed_case(world)
    ref, raw, _ = sc.reference(case)
    own, rs, inp = sc.block_owners(case, raw, world)
    con, nbytes, stride = sc.restate_contributions(ref, own, world)
    one = one_call(product, hip, dll, case, world, knobs=((ot.KNOB_SHARD_CHUNK_BYTES, knob),) if knob else ())
    all_equal(one["results"], ref, case["name"])
    assert not exchange_holds(one, ref, own, world, case["name"], knob)                     # every rank sends raw chunks of its padded contribution


# ---- D: the same cases through the multi-device ommCpuBake ----
def d_cases(devices):
    out = [sc.o_case("tiny", devices), sc.o_case("world", devices), sc.l_case("few", ot.FMT_2STATE), sc.l_case("few", ot.FMT_4STATE), sc.mixed_case(devices)]
    return out + [sc.u_case(f, le, gt) for f in tc.FORMATS for le, gt in sc.U_STATES[f]]


@pytest.mark.parametrize("devices", [2, 3, 8])
def test_multi_device_bake(product, devices):
    for case in d_cases(devices):
        ref = sc.reference(case)[0]
        got = {}

        def inspect(b):
            got["devices"] = timings(product, b).devices
        r = tc.bake(product, case, knobs=((ot.KNOB_DEVICES, devices),), inspect=inspect)
        assert r.same_as(ref), (case["name"], r.diff(ref))
        assert got["devices"] == devices, (case["name"], got)
