"""The 32-bit record offsets of the traversal's per-lane fetches (crt_device.h: pair_record, tri_hot_record, tri_cold_record, big_leaf_count,
instance_record) rest on the pools' fixed capacities. Each helper has a static_assert; this test says the same in a sentence, from the sources:
the limits of include/crt_types.h, the pool sizes crt_device.h derives from them (CRT_TRI_POOL_SLOTS, CRT_NODE_POOL_SLOTS,
CRT_PAIR_POOL_RECORDS), and crt_upload.h's alloc_pools, which must allocate with those names and with the multipliers the bounds below use.
A later change of a capacity, of a record size or of an allocation fails here first."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = open(os.path.join(ROOT, "include", "crt_types.h")).read()
DEVICE = open(os.path.join(ROOT, "clraytracer_amd", "csrc", "crt_device.h")).read()
UPLOAD = open(os.path.join(ROOT, "clraytracer_amd", "csrc", "crt_upload.h")).read()
LIMIT = 1 << 32


def limit(name):
    return int(re.search(rf"\b{name}\s*=\s*(\d+)", TYPES).group(1))


def define(name):
    """the replacement text of `#define name ...` in crt_device.h, comment stripped"""
    return re.search(rf"^#define {name} (.*?)\s*(?://.*)?$", DEVICE, re.M).group(1)


def pool_sizes():
    tris, nodes = define("CRT_TRI_POOL_SLOTS"), define("CRT_NODE_POOL_SLOTS")
    m = [re.fullmatch(r"\(\(size_t\)CRT_MAX_TRIANGLES \* (\d+)\)", x) for x in (tris, nodes)]
    assert all(m), (tris, nodes)
    assert define("CRT_PAIR_POOL_RECORDS") == "(CRT_NODE_POOL_SLOTS / 2 + 1)"
    tri_slots, node_slots = (limit("CRT_MAX_TRIANGLES") * int(x.group(1)) for x in m)
    return tri_slots, node_slots, node_slots // 2 + 1


def record_bytes(name):
    return int(define(name).rstrip("u"))


def test_alloc_pools_allocates_with_the_constants_the_helpers_are_proven_with():
    body = UPLOAD[UPLOAD.index("int alloc_pools()"):UPLOAD.index("int read_environment()")]
    assert re.search(r"g\.triCap = CRT_TRI_POOL_SLOTS;", body) and re.search(r"g\.nodeCap = CRT_NODE_POOL_SLOTS;", body)
    for pool, size in (("pairs", "(g.nodeCap / 2 + 1) * 4"), ("triHot", "g.triCap * 9"), ("triCold", "g.triCap * 2"), ("bigLeaf", "g.triCap + 1")):
        assert f"g.{pool}.alloc({size})" in body, f"alloc_pools no longer allocates {pool} as {size}: the bounds of this test are about another pool"
    # nothing else assigns the capacities
    assert len(re.findall(r"g\.(triCap|nodeCap)\s*=[^=]", UPLOAD)) == 2
    slots = re.search(r"fs\.devInstances\.alloc\((\w+)\)", UPLOAD).group(1)
    assert slots == "CRT_MAX_INSTANCES"


def test_every_helper_s_largest_byte_offset_is_below_2_to_the_32():
    tri_slots, node_slots, pair_records = pool_sizes()
    assert (tri_slots, node_slots) == (2400000, 2400000)          # today's pools (ResourceManager.cpp:158-159): a change is deliberate
    pair, hot, cold = record_bytes("CRT_PAIR_BYTES"), record_bytes("CRT_TRI_HOT_BYTES"), record_bytes("CRT_TRI_COLD_BYTES")
    assert (pair, hot, cold) == (64, 36, 32)
    # the largest index each helper can be handed (upload validation, crt_relayout.h make_ref): a pair index below the pool's records; a
    # triangle index up to the pool's slots inclusive -- the empty reference names slot `triCap`, whose address is formed and never loaded
    # from, and whose bigLeaf entry exists (alloc_pools: triCap + 1); a hit's triangle below the slots; an instance below CRT_MAX_INSTANCES
    largest = {
        "pair_record": (pair_records - 1) * pair,
        "tri_hot_record": tri_slots * hot,
        "tri_cold_record": (tri_slots - 1) * cold,
        "big_leaf_count": tri_slots * 4,
        "instance_record": (limit("CRT_MAX_INSTANCES") - 1) * 64,
    }
    for helper, offset in largest.items():
        assert re.search(rf"\b{helper}\(", DEVICE), helper
        assert offset < LIMIT, f"{helper}: a byte offset of {offset} no longer fits 32 bits -- the pool has outgrown TR_OFFSET32 (crt_device.h)"
    # the leaf reference's own field is narrower than the pool could grow: firstTri has 24 bits, and even its largest value times 36 fits
    assert (0x00FFFFFF + 127) * hot < LIMIT
    # the figures the design document quotes
    assert tri_slots * hot == 86_400_000 and (pair_records - 1) * pair == 76_800_000


def test_every_helper_has_its_static_assert_and_the_switch_exists():
    for text in ("CRT_PAIR_POOL_RECORDS * CRT_PAIR_BYTES < (1ull << 32)", "(CRT_TRI_POOL_SLOTS + 1) * CRT_TRI_HOT_BYTES < (1ull << 32)",
                 "CRT_TRI_POOL_SLOTS * CRT_TRI_COLD_BYTES < (1ull << 32)", "(CRT_TRI_POOL_SLOTS + 1) * sizeof(uint32_t) < (1ull << 32)",
                 "(size_t)CRT_MAX_INSTANCES * sizeof(CrtDevInstance) < (1ull << 32)"):
        assert f"static_assert({text}" in DEVICE, text
    assert "#ifdef CRT_NO_OFFSET32" in DEVICE and "TR_OFFSET32" in DEVICE
