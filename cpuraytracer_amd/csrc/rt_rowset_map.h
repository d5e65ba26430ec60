// rt_rowset_map.h -- where a row of the image lies under a cyclic row set (include/rt_api.h rt_rowset): the inverse of
// rt_rowset_global_row.  Integer arithmetic only, written once and compiled for the device (rt_denoise.hip, the prepare pass that
// reads the gathered parts of the shards) and for the host (host/rt_denoise_host.cpp: rt_rowset_locate, rt_unit_denoise_shards_host).
#pragma once

#include <stdint.h>

#include "rt_device_math.h"

namespace rtd {

// Row j of the row range (counted from its first row) is row k of block b = j / block_rows; blocks go to the shards in turn, so the
// block is shard b % nshards's local block b / nshards.  block_rows, nshards > 0.
RT_DEV void rowset_locate(uint32_t block_rows, uint32_t nshards, uint32_t j, uint32_t& shard, uint32_t& local_row) {
    const uint32_t b = j / block_rows, k = j - b * block_rows;
    const uint32_t lb = b / nshards;
    shard = b - lb * nshards;
    local_row = lb * block_rows + k;
}

// Rows shard `shard` owns of num_rows rows (what rt_rowset_local_rows counts block by block): its blocks are full but for the last
// block of the range, which is short where block_rows does not divide num_rows.  block_rows, nshards > 0.
RT_DEV uint32_t rowset_shard_rows(uint32_t num_rows, uint32_t block_rows, uint32_t nshards, uint32_t shard) {
    const uint64_t nblocks = ((uint64_t)num_rows + block_rows - 1u) / block_rows;
    if (shard >= nshards || nblocks <= shard) return 0;
    const uint64_t mine = (nblocks - shard + nshards - 1u) / nshards;
    uint64_t rows = mine * block_rows;
    const uint32_t tail = num_rows % block_rows;
    if (tail != 0 && (nblocks - 1u) % nshards == shard) rows -= block_rows - tail;
    return (uint32_t)rows;
}

// The largest shard's rows: what a part of the equal-count gather must hold.  That is shard 0's: no shard has more blocks, and a
// shard with as many has its last block after shard 0's last, so shard 0's blocks are all full.
RT_DEV uint32_t rowset_max_shard_rows(uint32_t num_rows, uint32_t block_rows, uint32_t nshards) {
    return rowset_shard_rows(num_rows, block_rows, nshards, 0);
}

}  // namespace rtd
