"""The launch shapes of the split suffix attention's exact checks and the turn-2 prompt of the prefix-session tests: one list
for tests/test_suffix_cpu.py (the oracle's conditions, no GPU), tests/test_suffix_gpu.py, tests/test_prefix_gpu.py and their
child process.  The smallest shapes that cross a wave (16 queries), a tile (64 keys), a split range and the cache's end."""
from tests import attention_oracle as AO
from tests import golden_cfg as G


def C(name, B, S, past, heads, ctx_max, **kw):
    return AO.Case(name, B, S, [past] * B, heads, ctx_max, **kw)


CASES = [
    C("s1_p0", 1, 1, 0, 2, 64),
    C("s64_p0_full", 1, 64, 0, 2, 64),
    C("s16_p1", 1, 16, 1, 2, 128),
    C("s17_p63", 1, 17, 63, 3, 128),
    C("s15_p64", 1, 15, 64, 2, 128),
    C("s33_p255", 1, 33, 255, 2, 320),
    C("s64_p256_full", 1, 64, 256, 2, 320),
    C("s48_p257_pad_holes", 1, 48, 257, 2, 384, pads=[9], holes=True),
    C("s2_p1023", 1, 2, 1023, 4, 1088),
    C("s63_p1024", 1, 63, 1024, 4, 1088, stride_extra=5),
    C("b2_s31_p1000_pads_holes", 2, 31, 1000, 4, 1100, pads=[70, 0], holes=True, stride_extra=3),
    C("b3_s20_p100_pads", 3, 20, 100, 2, 128, pads=[0, 64, 9]),
    C("s9_p336_h40", 1, 9, 336, 40, 400),
    C("s64_p1500", 1, 64, 1500, 8, 2048, full_valid=True),
]
BY_NAME = {c.name: c for c in CASES}
DENSE = ["s33_p255", "b2_s31_p1000_pads_holes", "s64_p1500"]       # the three cases of the dense-data error comparison
FP16_CASE = "b2_s31_p1000_pads_holes"                              # the child process's case on the fp16 storage type (several splits)

# the conversation of tests/test_prefix_gpu.py: turn 1 is the "decode2" fixture (283 tokens, its 8 greedy tokens pinned by
# g5_decode2.npz); turn 2 appends the first 6 of them and 40 further text tokens (329 tokens)
TURN1_NEW = 8
TURN2_KEEP = 6
TURN2_TEXT = ("turn2.1140", 40)
TURN2_TOKENS = [12, 278, 238, 163, 149, 6]
TURN2_MIN_GAP = 0.34


def turn2_ids(ids1, tokens1):
    """ids1: the turn-1 prompt (a list of ints); tokens1: its greedy continuation -> the turn-2 prompt."""
    return list(ids1) + list(tokens1[:TURN2_KEEP]) + G._text(*TURN2_TEXT)
