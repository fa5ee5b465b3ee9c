"""The summed-area table of `alpha > cutoff` that ommCpuCreateTexture builds on the device (bake_kernels.hip: sat_rows, sat_cols_block,
sat_cols_carry, sat_cols_add), read back through ommCpuSerialize and compared entry for entry with the numpy reference of
tests/sat_util.py -- no tolerance.  Whole bakes only ever ask the table "uniform below / uniform above / mixed" about the rectangles
their triangles happen to cover; here every entry of every mip is looked at, at the sizes where the kernels change path: the 64-texel
chunks and carried sum of the row pass, the 64-row blocks, 256-column workgroups and carry pass of the column pass.  Also pinned: the
layout of the section in both tilings (Morton-Z textures keep a row-major table in a slot sized for the padded square), zeroed slot
remainders, no section without a cut-off, dirty pooled scratch, and the deserializer's rebuild."""
import ctypes as C
import numpy as np
import pytest
import blobfmt
import ommtest as ot
import sat_util as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


@pytest.fixture(scope="module")
def xxh64(oracle):
    oracle.dll.orc_xxh64.restype = C.c_uint64
    oracle.dll.orc_xxh64.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64]
    return lambda dat, s: oracle.dll.orc_xxh64(dat, len(dat), s)


@pytest.mark.parametrize("w,h", su.shapes(), ids=["%dx%d" % s for s in su.shapes()])
def test_sat_every_entry(product, baker, w, h):
    """random / all above (last entry w * h, every carry in use) / all below / single texels above, both tilings, both compress flags; random in
    both texture formats, the rest in one (alternating with the shape)"""
    for disable_zorder in su.tilings(w, h):
        for fp32 in (False, True):
            for name, tex in su.contents(w, h, fp32, seed=w * 1000 + h):
                if name != "random" and fp32 != bool((w + h) & 1):
                    continue
                su.tables_of(product, baker, [tex], su.CUTOFF, disable_zorder)


@pytest.mark.parametrize("w,h", su.BIG_SHAPES, ids=["%dx%d" % s for s in su.BIG_SHAPES])
def test_sat_big_shapes(product, baker, w, h):
    """one row of 65 chunks, one column of 65 row blocks, and 17 x 17 blocks with ragged edges both ways (linear tiling)"""
    for fp32 in (False, True):
        for name, tex in su.contents(w, h, fp32, seed=w + h):
            if name == "random" or fp32 == bool(w & 1):
                su.tables_of(product, baker, [tex], su.CUTOFF, True)


@pytest.mark.parametrize("disable_zorder", [True, False])
def test_sat_fp32_special_values(product, baker, disable_zorder):
    """NaN (never above), +-inf, -0.0 against cut-off 0, texels equal to the cut-off and one ulp to either side, denormals"""
    for cutoff, tex in su.fp32_special_cases():
        su.tables_of(product, baker, [tex], cutoff, disable_zorder)


@pytest.mark.parametrize("disable_zorder", [True, False])
def test_sat_unorm8_cutoffs(product, baker, disable_zorder):
    """byte * (1 / 255) against cut-offs k * (1 / 255), one ulp to either side, 0 and 1: every byte value in every column phase of a chunk"""
    tex = ((np.arange(65)[None, :] * 7 + np.arange(67)[:, None] * 13) % 256).astype(np.uint8)
    assert np.unique(tex).size == 256
    for cutoff in su.unorm8_cutoffs():
        su.tables_of(product, baker, [tex], cutoff, disable_zorder)


@pytest.mark.parametrize("disable_zorder", [True, False])
@pytest.mark.parametrize("fp32", [False, True])
def test_sat_mips_of_unrelated_sizes(product, baker, xxh64, disable_zorder, fp32):
    """257x129, 64x65, 1x1 in one texture: slot offsets (64-byte aligned, padded squares under Morton-Z), each table, zero remainders; digest checked"""
    mips = [su.contents(w, h, fp32, seed=9 + w)[0][1] for (w, h) in [(257, 129), (64, 65), (1, 1)]]
    su.tables_of(product, baker, mips, su.CUTOFF, disable_zorder, xxh64=xxh64)
    mips = [su.contents(w, h, fp32, seed=9 + w)[1][1] for (w, h) in [(257, 129), (64, 65), (1, 1)]]
    su.tables_of(product, baker, mips, su.CUTOFF, disable_zorder, xxh64=xxh64)


@pytest.mark.parametrize("disable_zorder", [True, False])
def test_no_cutoff_no_table(product, baker, disable_zorder):
    tex = su.contents(65, 63, False, seed=1)[0][1]
    su.tables_of(product, baker, [tex], -1.0, disable_zorder)
    su.tables_of(product, baker, [tex, tex[:5, :3]], -1.0, disable_zorder)


def test_sat_scratch_block_reused_dirty(product):
    """The column pass keeps its block totals in a pooled scratch block that is handed out as it was left.  Textures of different sizes back to
    back on one baker, all above the cut-off (the largest totals) before random ones; textures alive together, tables read afterwards."""
    b = product.create_baker()
    alive = []
    for n, (w, h, kind) in enumerate([(513, 257, 1), (300, 129, 0), (257, 257, 0), (64, 65, 1), (513, 257, 0), (1, 200, 0)]):
        tex = su.contents(w, h, False, seed=40 + n)[kind][1]
        alive.append((tex, product.create_texture(b, [tex], alpha_cutoff=su.CUTOFF, disable_zorder=True)))
    for tex, t in alive:
        parsed = blobfmt.parse_blob(su.serialize_texture(product, b, t, 0))
        su.check_tables(parsed["inputs"][0]["texture"], [tex], su.CUTOFF, True)
    for tex, t in alive:
        product.destroy_texture(b, t)
    product.destroy_baker(b)


@pytest.mark.parametrize("compress", [0, 1])
@pytest.mark.parametrize("disable_zorder", [True, False])
def test_sat_survives_the_deserializer(product, baker, compress, disable_zorder):
    """blob -> ommCpuDeserialize (which builds the table again) -> ommCpuSerialize of the deserialized input: the same texture payload, table included"""
    su.bind(product.dll)
    mips = [su.contents(w, h, False, seed=70 + w)[0][1] for (w, h) in [(129, 65), (63, 200)]]
    blob = su.tables_of(product, baker, mips, 0.3, disable_zorder, compress_modes=(compress,))
    buf = C.create_string_buffer(blob, len(blob))
    bd = su.BlobDesc(C.cast(buf, C.c_void_p), len(blob))
    h = C.c_void_p()
    assert product.dll.ommCpuDeserialize(baker, C.byref(bd), C.byref(h)) == ot.SUCCESS
    pd = C.POINTER(su.DeserializedDesc)()
    assert product.dll.ommCpuGetDeserializedDesc(h, C.byref(pd)) == ot.SUCCESS
    assert pd.contents.numInputDescs == 1 and pd.contents.numResultDescs == 0
    again = su.serialize_inputs(product, baker, [pd.contents.inputDescs[0]], compress)
    assert product.dll.ommCpuDestroyDeserializedResult(h) == ot.SUCCESS
    t0, t1 = (blobfmt.parse_blob(x)["inputs"][0]["texture"] for x in (blob, again))
    su.check_tables(t1, mips, 0.3, disable_zorder)
    assert t1["sat_size"] == t0["sat_size"] and t1["mip_descs"] == t0["mip_descs"]
    for m in range(2):
        assert np.array_equal(t0["sat"][m], t1["sat"][m]) and t0["sat_rest"][m] == t1["sat_rest"][m]
    assert again == blob
