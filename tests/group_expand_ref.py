"""numpy restatement of ``afcm_group_expand`` (include/afcm_hip.h; kernel in afcm_amd/csrc/group.hip): whole per-sample blocks of raw bytes,
``out[b] = in[groups[b]]``, and a block of NaN elements for every index outside [0, G).  The GPU tests (tests/test_gpu_group_expand.py) compare the
kernel's bytes with these; tests/test_group_expand_ref_cpu.py holds the restatement itself to ``np.take``."""
import numpy as np

# the element patterns the kernel stores for an invalid index, by element size (0x7FFF is a NaN in float16 and in bfloat16)
NAN_BITS = {2: np.uint16(0x7FFF), 4: np.uint32(0x7FC00000)}


def expand_bytes(src, block_bytes, groups, elem_size):
    """``src``: uint8 array of G * block_bytes bytes (the tensor as allocated, padding included); ``groups``: int array [B].  Returns
    (uint8 [B, block_bytes], bool [B] -- True where the index is invalid and the block is NaN elements)."""
    src = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
    assert block_bytes > 0 and block_bytes % elem_size == 0 and src.size % block_bytes == 0
    blocks = src.reshape(-1, block_bytes)
    g = np.asarray(groups, dtype=np.int64)
    invalid = (g < 0) | (g >= blocks.shape[0])
    out = np.empty((g.size, block_bytes), dtype=np.uint8)
    nan_block = np.full(block_bytes // elem_size, NAN_BITS[elem_size]).view(np.uint8)
    for b in range(g.size):
        out[b] = nan_block if invalid[b] else blocks[g[b]]
    return out, invalid


def chunks(block_bytes_list, batch, chunk_bytes):
    """(chunk0 of every row, total) as the Python op lays the table out: row k owns batch * ceil(block_bytes / chunk_bytes) chunks."""
    firsts, total = [], 0
    for bb in block_bytes_list:
        firsts.append(total)
        total += batch * (-(-bb // chunk_bytes))
    return firsts, total


# (elements per block) by element size: below, at and above one 16-byte access, with a tail, and a block that crosses a workgroup's 16 KiB chunk
BLOCK_ELEMS = {2: (1, 7, 8, 8 * 5 + 3, 8 * 1024 + 8 * 3 + 3), 4: (1, 3, 4, 4 * 5 + 1, 4 * 1024 + 4 * 3 + 1)}

# name -> (G, groups): G = 1 with B = 5; G > B; non-monotone with repeats; -1 and G in the first and the last sample
INDEX_CASES = {
    'one_group': (1, [0, 0, 0, 0, 0]),
    'more_groups_than_samples': (7, [6, 2, 4]),
    'non_monotone_repeats': (4, [3, 0, 3, 1, 1, 0, 2, 3]),
    'invalid_first_and_last': (3, [-1, 2, 0, 1, 3]),
    'invalid_last_and_first': (3, [3, 1, 1, -1]),
}
