/* latticenet_hip.h — C ABI of the MI355X (gfx950) permutohedral-lattice backend.
 *
 * Drop-in boundary for ONE path of AIS-Bonn/lattice_net: everything `latticenet.Lattice`
 * (src/PyBridge.cxx:41-113) forwards to `LatticeGPU` launch wrappers
 * (include/lattice_net/kernels/LatticeGPU.cuh:42-412).  Each entry point below names the
 * reference interface it replaces.  Plain C: device pointers, sizes, a stream handle
 * (hipStream_t passed as void*), int status.  No torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - all tensors are contiguous row-major; positions/values/weights fp32, indices int32;
 *   - return value 0 = launched OK; <0 = argument / launch error, text via
 *     ln_last_error_string(); kernels never block the host;
 *   - asynchronous device-side conditions (table full, key out of packable range) are
 *     recorded in LnTable.status and must be read back by the caller (ln_status_string).
 *
 * Vertex numbering: deterministic.  Builds that start from a cleared table number the vertices bucket by bucket
 * (runs of consecutive hash slots; inside a bucket by first occurrence) — the reference's own numbering is thread-arrival
 * order and not reproducible; with
 * LN_BUILD_CANONICAL_ROWS / ln_canonicalize, and on every incremental build, rows are numbered by first
 * occurrence in (point, remainder) order, i.e. what a serial run of HashTableGPU::insert
 * (HashTableGPU.cuh:425-484) produces.
 */
#ifndef LATTICENET_HIP_H
#define LATTICENET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LN_OK 0
#define LN_ERR_ARG (-1)
#define LN_ERR_UNSUPPORTED (-2)
#define LN_ERR_LAUNCH (-3)
#define LN_ERR_WORKSPACE (-4)

/* bits of *LnTable.status (device int32) */
#define LN_STATUS_TABLE_FULL 1      /* insert probed every slot (reference would spin forever, HashTableGPU.cuh:443) */
#define LN_STATUS_KEY_RANGE 2       /* a lattice key did not fit the packed 64-bit slot format */
#define LN_STATUS_BUCKET_OVERFLOW 4 /* bucketed build: one LDS-staged bucket filled up; nothing of this build is valid,
                                       re-run it with LN_BUILD_ATOMIC_PATH (whose inserts spill past a full bucket) */
#define LN_STATUS_CLOUD_BAND 8      /* a cloud of a batch leaves its key band (set by ln_cloud_key_extents, never by a build) */
#define LN_STATUS_CLOUD_STARTS 16   /* LnTableClouds.batch_point_starts is not an ascending list from 0 to n (set by ln_cloud_point_starts_check) */

#define LN_MAX_POS_DIM 6
#define LN_SLOT_MAP_INTS 32 /* ints behind LnTable.slot_map */
#define LN_KEYS_RAW 0     /* LnTable.key_format */
#define LN_KEYS_LATTICE 1
#define LN_NOT_VISITED (-2)          /* neighbour-list code: traversal never looks at this slot */

/* Device-side open-addressing table.  Replaces HashTableGPU (HashTableGPU.cuh:12-30) and its
 * host owner HashTable (src/HashTable.cu:21-47).  `keys`, `entries`, `nr_filled` have exactly
 * the reference's meaning and layout; `slot_keys`/`slot_tok`/`status` are additions:
 *   slot_keys[h]  the lattice key stored in slot h, packed into 64 bits (all-ones = empty), so
 *                 claim + key publication is ONE 64-bit CAS (no spin lock, no fence);
 *   slot_tok[h]   smallest insertion token that touched slot h during the build that created
 *                 it (0xFFFFFFFF while empty) — defines the canonical row order;
 *   slot_cnt[h]   how many tokens of the current build landed on slot h;
 *   status        sticky error bits, see LN_STATUS_*. */
typedef struct LnTable {
    int capacity;
    int pos_dim;
    unsigned long long* slot_keys; /* [capacity] */
    unsigned int* slot_tok;        /* [capacity] */
    int* slot_cnt;                 /* [capacity] tokens of the current build per slot (scratch) */
    int* entries;                  /* [capacity]   slot -> row, -1 empty  (m_entries) */
    int* keys;                     /* [capacity,d] row  -> key            (m_keys)    */
    int* nr_filled;                /* [1]                                 (m_nr_filled) */
    int* status;                   /* [1] */
    int* host_counters;            /* NULL, or 8-byte aligned pinned, device-visible host memory: every build ends with ONE 64-bit store
                                      there: nr_filled | status << 32 | (host_seq & 0xFFFFFF) << 40.  A host that passes a fresh
                                      host_seq per build can spin on that word and read the vertex count as soon as the build's last
                                      kernel has got there, without a copy or an event */
    int host_seq;                  /* sequence number of this build (24 bits are reported) */
    int key_format;                /* how slot_keys packs a key (fixed for the life of the table's contents): 0 = raw, any integer
                                      tuple (needed by ln_coarsen's target, which receives halved fine keys); 1 = lattice points
                                      only — remainder + quotients, 6-7x the coordinate range for pos_dim 5-6 (every table
                                      built from positions).  See KeyPack in csrc/ln_common.h */
    int row_limit;                 /* 0 = none.  > 0 (static-rows mode of the host, whose [rows, *] tensors are this tall): a build
                                      leaves vertices that would get a row >= row_limit un-inserted — idx = -1, no entries[] /
                                      keys[] row — so that no consumer can index past the host's tensors; nr_filled still
                                      counts them, which is how the host notices (nr_filled > row_limit) */
    const int* slot_map;           /* NULL (slots hashed over the whole table, as the reference), or LN_SLOT_MAP_INTS device ints that
                                      order the SLOTS — and with them the rows — of this table by space:
                                        [0..6]   planes of a 3-level kd partition of KEY space into 8 leaves, heap order (node i has the
                                                 children 2i+1: key below the plane, 2i+2: key >= plane; level l compares key[l % pos_dim]);
                                        [7]      buckets per leaf = ln_table_bucket_count(capacity) / 8;
                                        [8..16]  first slot of each leaf's run of slots, then the end of the last run (<= capacity);
                                        [17..24] slots per bucket inside each leaf (run length = [7] x this).
                                      A key starts probing inside its leaf's run (the hash picks the slot), rows are numbered bucket by
                                      bucket, so the vertices of a leaf own one contiguous row range and the gathers of the path (9
                                      neighbour rows per vertex, d+1 rows per point) stay inside one XCD's L2.  The map must stay what it
                                      was when the table's contents were inserted (retrieval uses the same function): change it only in
                                      front of a build that starts with a clear.  A map whose leaves do not fit the cloud overfills
                                      buckets (LN_STATUS_BUCKET_OVERFLOW -> rebuild on the atomic path, whose inserts spill); a fitting
                                      one comes from the host's calibration (Lattice.balanced_region_planes).  csrc/ln_common.h */
    int bucket_slots_max;          /* with a slot map: the largest of its slots-per-bucket entries (sizes the LDS of the bucket pass) */
    int batch_points;              /* 0, > 0, or LN_BATCH_POINT_STARTS (clouds of unequal sizes, see LnTableClouds below).  > 0: the positions handed to a build / retrieval of this table are a BATCH of independent clouds
                                      of batch_points points each (cloud c = point index / batch_points).  Cloud c's lattice keys are then
                                      shifted by c * batch_key_step on the first coordinate — a multiple of pos_dim + 1, i.e. a translation
                                      of the lattice onto itself — so that the clouds' vertex sets are disjoint in ONE table and every kernel
                                      of the path (neighbour lists, convolutions, slice, the scatters) runs over the batch in one launch with
                                      per-cloud results (the multi-cloud launch form for clouds too small to fill the chip) */
    int batch_key_step;            /* (pos_dim + 1) x the quotient distance between clouds; halved per coarser level so that the
                                      level-crossing neighbour search (keys x 2^(lvl difference)) stays inside a cloud */
    int* row_regions;              /* NULL, or LN_XCD_GROUPS + 1 device ints a bucketed build over a space-ordered table fills: the first row
                                      of each of the 8 top-level kd regions and the row count — the `row_partition` argument of the convolutions */
} LnTable;

/* A batch of clouds of UNEQUAL sizes: an LnTable with a tail.  LnTable itself keeps its layout; a table whose batch_points is
 * LN_BATCH_POINT_STARTS is the first member of an LnTableClouds, and every entry point that takes the cloud of a point from the table
 * (ln_build_splat, ln_distribute, ln_slice_no_precomputation, ln_cloud_key_extents) reads the tail: pass &clouds.table.  Any other
 * batch_points (0: no batch, > 0: equal sizes) means a plain LnTable, nothing behind it is read, and everything is what it was.
 *   batch_point_starts  batch_clouds + 1 device ints: ascending, starts[0] = 0, starts[batch_clouds] = n; cloud c is the points
 *                       [starts[c], starts[c + 1]) and may be empty.  The cloud of point p is upper_bound(starts, p) - 1, found by a
 *                       binary search (csrc/ln_simplex.h); batch_key_step keeps its meaning.  A kernel only compares against these ints
 *                       and clamps what it takes from them to [0, n]: a list that breaks the rules gives wrong clouds, never an access
 *                       out of bounds (ln_cloud_point_starts_check tells).
 *   batch_clouds        >= 1.
 * A null list or batch_clouds < 1 behind LN_BATCH_POINT_STARTS is LN_ERR_ARG, nothing launched. */
#define LN_BATCH_POINT_STARTS (-1) /* LnTable.batch_points: the sizes come from the LnTableClouds this table heads */
typedef struct LnTableClouds {
    LnTable table;
    const int* batch_point_starts;
    int batch_clouds;
} LnTableClouds;

/* Adjacency "group -> the tokens that touch it" in CSR form, cut into segments of at most 16
 * entries (the unit of work of ln_csr_reduce_rows).  A group is a hash slot for the CSR that
 * ln_build_splat / ln_distribute / ln_coarsen emit as a by-product (row of a group = entries[slot]),
 * or a row for ln_csr_build (row of a group = the group). */
#define LN_XCD_GROUPS 8 /* segment / point / vertex lists are kept per XCD group (see csrc/ln_common.h, LnProbe) */
typedef struct LnCsr {
    int* grp_start; /* [groups_upper + 1] */
    int* csr_tok;   /* [tokens]           tokens grouped by group */
    int* seg_desc;  /* [LN_XCD_GROUPS * seg_region * 4], 16-byte aligned: one descriptor {group, first CSR entry, entries from
                       there to the end of the group, offset of the first entry inside the group} per segment — everything a
                       reduce needs about a segment in ONE 16-byte load; region g holds the segments of XCD group g */
    int* seg_count; /* [LN_XCD_GROUPS + 2] device-side number of segments per region, then the number of regions in use
                       (1: everything in region 0 — ln_csr_build, the atomic build path; LN_XCD_GROUPS: bucketed build with
                       planes), then the descriptor format: 0 = the first descriptor word is the group; 1 (bucketed build) = it is the
                       ROW of the group, so a reduce needs no group -> row lookup */
    long long seg_region; /* entries per region (>= ln_csr_max_segments: one region may hold every segment) */
    const int* planes;    /* NULL (everything in region 0), or 7 device ints: split planes of a 3-level kd partition of KEY space
                             into LN_XCD_GROUPS compact regions — key[0] >= planes[0] picks the half, key[1] against
                             planes[1 + half] the quarter, key[2] against planes[3 + quarter] the region.  A bucketed
                             build then files every vertex's segments under its region, and the scatter kernels let
                             XCD r walk region r: the d+1 gathers of a point row meet in ONE L2.  These planes only steer
                             work placement (any values are correct).  When the table itself is space-ordered
                             (LnTable.slot_map) the region of a vertex is that of its bucket and this array is only a flag. */
    int dense;            /* host-side hints for the segment reduces (any value is correct).  Bit 0 = dense cloud, about 16 or more
                             tokens per vertex — most vertices then own several segments, and the reduce combines partial sums across
                             the waves of a workgroup before it resorts to atomics (C5: 104 -> 84 us; costs the sparse C3 scan 10 %).
                             Bit 1 = deterministic: one lane group walks a whole row in CSR order and stores it — no atomics, no
                             combining; with LN_BUILD_SORTED_CSR the sums are identical run to run (slower on hot vertices) */
} LnCsr;

const char* ln_last_error_string(void);
const char* ln_version(void);
/* short hash of THIS header as it was when the library was built (the binding compares it with the header it was written
 * against and refuses a stale library) */
const char* ln_abi_hash(void);

/* Live per-kernel timing (used by bench.py for the roofline block).  ln_profile_begin arms timing of every launch of the
 * kernels named in `kernel_names` (one name of ln_kernel_names, or several separated by commas), up to max_samples launches in
 * total: each such launch carries a (start, stop) event pair bound to the dispatch itself (hipExtLaunchKernelGGL), i.e. the
 * kernel's own duration as rocprofv3 reports it.  ln_profile_end waits for the recorded pairs, returns the summed duration and
 * the number of launches, and disarms.  Launches inside a stream capture cannot be timed this way (do not arm across one). */
const char* ln_kernel_names(void);
int ln_profile_begin(const char* kernel_names, int max_samples);
int ln_profile_end(double* total_ms, int* launches);
/* The same with a breakdown: kernel_names "*" arms every launch of the library; ln_profile_end_table ends the profiling like
 * ln_profile_end and writes one line "name launches total_ms\n" per launch name that occurred (in order of first occurrence,
 * NUL-terminated, truncated to out_bytes) — bench.py's per-operator roofline table. */
int ln_profile_end_table(char* out, int out_bytes);

/* HashTable::clear (src/HashTable.cu:49-57): entries=-1, keys=0, nr_filled=0 (+ our slots/status)
 * in one launch.  `values` (may be NULL) is zero-filled too: values_elems floats. */
int ln_table_clear(const LnTable* t, float* values, long long values_elems, void* stream);

/* The freshly allocated structure buffers of a table in one launch (the reference's HashTable::init issues one fill per tensor,
 * src/HashTable.cu:21-47): `arena` holds `words` 32-bit words; words [minus_begin, minus_end) are set to -1 (the entries), every
 * other word to 0 (keys, slot counters, the device counters, a placeholder values row — carved from the arena by the host). */
int ln_arena_init(int* arena, long long words, long long minus_begin, long long minus_end, void* stream);

/* Buckets (runs of consecutive slots, one workgroup of the bucketed build each) of a table that hashes into `capacity` slots: what a
 * host needs to lay out LnTable.slot_map. */
int ln_table_bucket_count(int capacity);

/* Scratch needed by ln_build_splat / ln_distribute / ln_coarsen for `tokens` insertions. */
size_t ln_build_workspace_bytes(long long tokens, int capacity);

/* kernel_splat (LatticeGPU.cuh:707-842) behind Lattice::splat_standalone / just_create_verts
 * (src/Lattice.cu:196-290), with `positions_raw / sigmas` (Lattice.cu:226) fused in.
 * Inserts the d+1 simplex vertices of every point; when flags has LN_BUILD_WRITE_IDX writes
 * idx[n*(d+1)] (row ids) and w[n*(d+1)] (barycentric weights).  Both must be pre-sized; rows
 * that cannot be inserted keep -1 (Lattice.cu:212-215 semantics are produced here, no pre-fill
 * needed).  idx/w may be NULL without that flag.
 * `csr` (required; groups = hash slots, groups_upper = capacity, sized with ln_csr_max_segments)
 * receives the slot -> tokens adjacency of this build: the build needs it to find each vertex's
 * first occurrence, and the caller reuses it for every scatter onto the vertices
 * (ln_csr_reduce_rows with grp_row = t->entries).
 * flags: LN_BUILD_WRITE_IDX = write idx / w; LN_BUILD_CLEAR_FIRST = run ln_table_clear(t, clear_values,
 * clear_values_elems) first, in the same call (begin_splat + splat in one host round trip).
 * Two build paths produce the same table, rows, idx and CSR semantics:
 *   bucketed (taken when LN_BUILD_CLEAR_FIRST is set and LN_BUILD_ATOMIC_PATH is not): tokens are partitioned by
 *     hash bucket and each bucket is resolved by one workgroup in LDS, no per-token global atomics.  A bucket
 *     of ~512 slots that fills up (tables loaded beyond ~0.85) sets LN_STATUS_BUCKET_OVERFLOW.
 *   atomic (any table state, any load < 1): one 64-bit CAS per new vertex + one returning add per token. */
#define LN_BUILD_WRITE_IDX 1
#define LN_BUILD_CLEAR_FIRST 2
#define LN_BUILD_ATOMIC_PATH 4
#define LN_BUILD_CANONICAL_ROWS 8 /* bucketed path: run ln_canonicalize behind the build (the atomic path numbers canonically anyway) */
#define LN_BUILD_SORTED_CSR 16    /* rewrite every token list of `csr` in ascending token order behind the build: the order tokens arrive in
                                     differs from run to run, and with it the last bits of every fp32 sum over them.  With LnCsr.dense & 2
                                     in the reduces: run-to-run identical splat values / slice and gather gradients */
#define LN_BUILD_OVERLAPPED 32    /* the caller keeps several builds / scans in flight on this GPU.  A speed hint for this build: the bucket
                                     pass of a build over small buckets then runs on 512-thread workgroups, which finish a bucket later but
                                     pack beside the other scans' kernels (ln_table.hip).  No effect on results.  (The reference has no
                                     counterpart: its build is one stream's work, Lattice.cu:196-241.) */
int ln_build_splat(const LnTable* t, const float* positions_raw, const float* sigmas_host, int n, int* idx, float* w,
                   int flags, const LnCsr* csr, void* workspace, size_t workspace_bytes, float* clear_values,
                   long long clear_values_elems, void* stream);

/* Vertex numbering.  The reference numbers vertices in thread-arrival order (atomicAdd(m_nr_filled), HashTableGPU.cuh:454) — it
 * differs from run to run and nothing downstream depends on it.  The bucketed build numbers them bucket by bucket (inside a
 * bucket by the rank of the vertex's smallest token: deterministic, and the whole build is two launches).  ln_canonicalize relabels
 * the rows of a table that ONE bucketed build has just produced — entries[], keys[] and, when given, the idx[tokens] that
 * build wrote and the row ids in the segment descriptors of `csr` — into first-occurrence order over
 * (point, remainder), i.e. the numbering a serial run of HashTableGPU::insert (HashTableGPU.cuh:425-484) produces and the golden vectors hold.  It must run before anything that
 * stores row ids elsewhere (accumulated values, neighbour lists).  workspace: ln_build_workspace_bytes(tokens, capacity).
 * LN_BUILD_CANONICAL_ROWS makes ln_build_splat / ln_distribute do this themselves.
 * `csr` is the LnCsr that build filled: a bucketed build writes ROW ids into its segment descriptors, so it has to be relabelled
 * with the table.  Passing NULL is only valid when that CSR is never used again (the caller discards it): a scatter through the
 * stale descriptors would land on the old rows. */
int ln_canonicalize(const LnTable* t, int* idx, long long tokens, const LnCsr* csr, void* workspace, size_t workspace_bytes, void* stream);

/* A host may let a build hash into fewer slots than the table owns (LnTable.capacity = the slots in use: clearing and emitting
 * the slot range then costs what the cloud needs, not what the cfg's hash_table_capacity reserves — slot positions are not
 * reference-visible, only row ids are).  ln_rehash re-inserts the existing vertices (rows 0 .. nr_filled-1 of keys[]) into the
 * slot range [0, t->capacity) of the same buffers — call it with the larger capacity before an incremental build that may
 * outgrow the smaller range.  Rows, keys and counters are untouched. */
int ln_rehash(const LnTable* t, void* stream);

/* splatCacheNaive (LatticeGPU.cuh:926-973): table_values[idx] += vals * w. */
int ln_splat_accumulate(float* table_values, const float* vals, const int* idx, const float* w, int n, int pos_dim,
                        int val_dim, void* stream);

/* Scatter without per-element global atomics.  ln_csr_build transposes splat indices idx[tokens]
 * (row per token, <0 = skip) into an LnCsr whose groups are rows (groups_upper = rows_upper).
 * ln_csr_reduce_rows then ADDS, for every group g with row r = grp_row ? grp_row[g] : g,
 *     dst[r, j] += sum_{t in g} src[(t / src_div) * src_stride + j] * w[t],   j < val_dim
 * (dst zero-initialised by the caller): one lane group per segment, plain stores for groups that
 * fit one segment, global atomics only to combine the segments of longer ones.
 * With src_div = d+1, src_stride = V it replaces splatCacheNaive (LatticeGPU.cuh:926-973) and
 * slice_backwards_..._no_homogeneous (LatticeGPU.cuh:3540-3623); with src_div = 1,
 * src_stride = V+1 it replaces gather_backwards_with_precomputation (LatticeGPU.cuh:3761-3817). */
long long ln_csr_max_segments(long long tokens, int groups_upper);
size_t ln_csr_workspace_bytes(long long tokens, int groups_upper);
int ln_csr_build(const int* idx, long long tokens, int groups_upper, const LnCsr* csr, void* workspace, size_t workspace_bytes,
                 void* stream);
int ln_csr_reduce_rows(const LnCsr* csr, const int* grp_row, long long max_segments, const float* src, const float* w, int val_dim,
                       int src_div, int src_stride, float* dst, void* stream);
/* Rewrites every token list of a CSR (ln_csr_build's, or a build's: groups_upper = what it was built over) in ascending token order:
 * what LN_BUILD_SORTED_CSR does behind a build.  workspace: `tokens` ints (tokens = what the CSR was sized for). */
int ln_csr_sort(const LnCsr* csr, int groups_upper, void* workspace, size_t workspace_bytes, long long tokens, void* stream);

/* The two launches that follow a splat build and do not depend on each other, as ONE launch: ln_csr_reduce_rows(csr,
 * grp_row, .., dst) (splatCacheNaive) in the first workgroups, ln_neighbours(table, query_rows_upper, table, same level,
 * dilation 1, no flip, nbr) in the rest. */
int ln_splat_accumulate_and_neighbours(const LnCsr* csr, const int* grp_row, long long max_segments, const float* src, const float* w,
                                       int val_dim, int src_div, int src_stride, float* dst, const LnTable* table, int query_rows_upper,
                                       int* nbr, void* stream);

/* "Next" row: the vertex-wise aggregations PointNetModule runs on the distributed
 * rows — torch_scatter.scatter_max with argmax (lattice_modules.py:688) and scatter_add of ones
 * (lattice_modules.py:692) — on the same adjacency.
 * ln_csr_segment_max: out_max[r, c] = max over the tokens t of row r of src[t, c], out_arg[r, c] = the
 * token attaining it (smallest token on ties); rows without tokens get 0 / -1.
 * packed_ws: rows*channels*8 bytes of scratch.  ln_csr_group_sizes: counts[r] = tokens of row r. */
int ln_csr_segment_max(const LnCsr* csr, const int* grp_row, long long max_segments, const float* src, int channels, int rows,
                       void* packed_ws, float* out_max, int* out_arg, void* stream);
int ln_csr_group_sizes(const LnCsr* csr, const int* grp_row, int groups_upper, int rows, int* counts, void* stream);

/* distribute kernel (LatticeGPU.cuh:534-650) behind Lattice::distribute (Lattice.cu:351-410):
 * ln_build_splat + the dense rows [pos_scaled(d) | val(V) | bary] -> distributed[n*(d+1), d+V+1].
 * flags: LN_BUILD_CLEAR_FIRST / LN_BUILD_ATOMIC_PATH as for ln_build_splat (idx / w are always written). */
int ln_distribute(const LnTable* t, const float* positions_raw, const float* sigmas_host, const float* vals, int n,
                  int val_dim, int* idx, float* w, float* distributed, int flags, const LnCsr* csr, void* workspace,
                  size_t workspace_bytes, float* clear_values, long long clear_values_elems, void* stream);

/* coarsen kernel (LatticeGPU.cuh:2314-2514) behind Lattice::create_coarse_verts (Lattice.cu:670-703).
 * fine_rows_upper bounds the launch; the kernel also honours *fine->nr_filled. */
int ln_coarsen(const LnTable* fine, int fine_rows_upper, const LnTable* coarse, const LnCsr* csr, void* workspace,
               size_t workspace_bytes, void* stream);

/* Neighbour traversal shared by im2row / im2rowindices / row2im (LatticeGPU.cuh:1479-1684,
 * 1844-1915, 2187-2284): nbr[query_rows_upper, E] (E = 2(d+1)+1) rows of the neighbour table;
 * -1 = visited-but-absent, LN_NOT_VISITED = never looked at.  Slot layout as the reference:
 * axis a: np -> 2a+(flip), nm -> 2a+(1-flip); centre -> E-1. */
int ln_neighbours(const LnTable* query, int query_rows_upper, const LnTable* neigh, int lvl_query, int lvl_neigh,
                  int dilation, int flip, int* nbr, void* stream);

/* im2row (LatticeGPU.cuh:1464-1688) from a neighbour list: out[m, E*V]. */
int ln_im2row(const int* nbr, const float* values_neigh, int m, int filter_extent, int val_dim, float* out, void* stream);
/* im2rowindices (LatticeGPU.cuh:1690-1920): out[m, E*V] int32, reference fill rules. */
int ln_im2rowindices(const int* nbr, int m, int filter_extent, int val_dim, int* out, void* stream);
/* row2im (LatticeGPU.cuh:2067-2305): out[m, V] = adjoint gather of rowified[m_rows, E*V];
 * `nbr` is the un-flipped list of the OUTPUT lattice against the lattice indexing `rowified`. */
int ln_row2im(const int* nbr, const float* rowified, int m, int filter_extent, int val_dim, float* out, void* stream);

/* Lattice::convolve_im2row_standalone (Lattice.cu:424-474) without materialising the rowified
 * tensor: out[m, F] = sum_e values_neigh[nbr[m,e'], :] @ B_e   (fp32 MFMA), with
 *   flags & LN_CONV_FLIP_NEIGHBOURS   : e' = e^1 for the neighbour slots (what the reference's
 *        flip_neighbours traversal produces, LatticeGPU.cuh:1622-1626) — lets the backward pass reuse
 *        the forward neighbour list;
 *   flags & LN_CONV_TRANSPOSED_FILTER : `filter` is the [E*F, V] bank of the convolution being
 *        differentiated and B_e is its per-slot transpose, i.e. the filter_bank_backwards of
 *        lattice_funcs.py:307-311 without building it; otherwise `filter` is [E*V, F] and
 *        B_e = filter[e*V:(e+1)*V, :].
 * filter_extent = 1 with nbr = 0..m-1 is a per-vertex linear layer (the 1x1 blocks of lattice_modules.py:806-832):
 * out = values @ W^T for W = `filter` [F, V] under LN_CONV_TRANSPOSED_FILTER. */
#define LN_CONV_FLIP_NEIGHBOURS 1
#define LN_CONV_TRANSPOSED_FILTER 2
/* ln_conv_forward_ws only: the first ln_conv_bank_workspace_bytes(...) bytes of `workspace` still hold what an earlier call with the
 * SAME filter contents, sizes (m, filter_extent, val_dim, nr_filters) and flags left there (the filter split into bf16 parts in the
 * layout of the kernel those sizes select): the split launch is skipped.  For hosts that convolve repeatedly with unchanged
 * weights (inference; several clouds per optimizer step) and keep one workspace per layer. */
#define LN_CONV_BANK_READY 4
/* The caller keeps several scans in flight on this GPU (the meaning of LN_BUILD_OVERLAPPED).  A speed hint only: the fused 32-channel
 * kernels (filter_extent 9, val_dim = nr_filters = 32) then run as narrow workgroups that loop over their rows and leave room on
 * their CU for the other scans' kernels.  Same output, bit for bit; same workspace sizes.  Accepted by ln_conv_forward,
 * ln_conv_forward_ws and ln_conv_backward_flags. */
#define LN_CONV_OVERLAPPED 8
int ln_conv_forward(const int* nbr, const float* values_neigh, const float* filter, int m, int filter_extent, int val_dim,
                    int nr_filters, int flags, float* out, void* stream);
/* ln_conv_forward with scratch.  When the lattice has few vertices (coarse levels of a U-Net: fewer vertex tiles than CUs) the
 * contraction is split over the filter slots and the partial sums are added by a second launch; that needs
 * ln_conv_forward_workspace_bytes(m, filter_extent, val_dim, nr_filters) bytes of 16-byte aligned scratch (256 when no
 * split applies).  Without enough scratch it runs unsplit, exactly as ln_conv_forward.
 * `row_partition` (may be NULL): work placement hint for the vertex-tiled kernels — LnTable.row_regions of the space-ordered table whose
 * rows this call convolves over (device memory, 9 ints, read by the kernels at run time).  XCD x then works on the row tiles of kd
 * region x, whose neighbour rows share its L2.  Purely a speed matter: any contents give correct results. */
size_t ln_conv_bank_workspace_bytes(int m, int filter_extent, int val_dim, int nr_filters); /* the split-bank part (0: no split bank for these sizes) */
size_t ln_conv_forward_workspace_bytes(int m, int filter_extent, int val_dim, int nr_filters);
int ln_conv_forward_ws(const int* nbr, const float* values_neigh, const float* filter, int m, int filter_extent, int val_dim,
                       int nr_filters, int flags, float* out, void* workspace, size_t workspace_bytes, const int* row_partition, void* stream);
/* grad_filter = rowified^T @ grad_out (lattice_funcs.py:302) without the rowified tensor.
 * workspace: ln_conv_grad_filter_workspace_bytes(). */
size_t ln_conv_grad_filter_workspace_bytes(int m, int filter_extent, int val_dim, int nr_filters);
int ln_conv_grad_filter(const int* nbr, const float* values_neigh, const float* grad_out, int m, int filter_extent,
                        int val_dim, int nr_filters, float* grad_filter, void* workspace, size_t workspace_bytes,
                        void* stream);

/* slice_with_precomputation (LatticeGPU.cuh:2552-2595). */
int ln_slice_forward(const float* values, const int* idx, const float* w, int n, int pos_dim, int val_dim, float* out,
                     void* stream);
/* ln_slice_forward that also zero-fills `grad_accumulator` (grad_accumulator_elems floats): the [rows, val_dim] buffer the
 * backward pass of this slice scatters into (ln_csr_reduce_rows / ln_slice_backward need it zeroed), saving that fill launch. */
int ln_slice_forward_prepare_backward(const float* values, const int* idx, const float* w, int n, int pos_dim, int val_dim, float* out,
                                      float* grad_accumulator, long long grad_accumulator_elems, void* stream);
/* slice_with_precomputation for the indices a build of `t` wrote, with the points taken in the order of that build's slot CSR (`csr`,
 * as ln_build_splat / ln_distribute filled it; groups = hash slots) instead of input order: over a space-ordered table
 * (LnTable.slot_map) the d+1 value rows of the points a workgroup slices then sit in one kd region, i.e. in one XCD's L2.  Same
 * arithmetic per point, bit-identical output rows.  grad_accumulator (may be NULL) as ln_slice_forward_prepare_backward.  Widths the
 * ordered kernel does not cover run ln_slice_forward. */
int ln_slice_forward_ordered(const LnTable* t, const LnCsr* csr, const float* values, const int* idx, const float* w, int n, int val_dim,
                             float* out, float* grad_accumulator, long long grad_accumulator_elems, void* stream);

/* slice_no_precomputation (LatticeGPU.cuh:2598-2750): also writes idx/w (-1 where absent). */
int ln_slice_no_precomputation(const LnTable* t, const float* values, const float* positions_raw, const float* sigmas_host,
                               int n, int val_dim, float* out, int* idx, float* w, void* stream);
/* slice_backwards_with_precomputation_no_homogeneous (LatticeGPU.cuh:3540-3623);
 * grad_values[m_rows, V] must be zeroed by the caller (Lattice.cu:1079). */
int ln_slice_backward(const float* grad_sliced, const int* idx, const float* w, int n, int pos_dim, int val_dim,
                      float* grad_values, void* stream);

/* gather_with_precomputation (LatticeGPU.cuh:2886-2929): out[n, (d+1)(V+1)] (fully written). */
int ln_gather_forward(const float* values, const int* idx, const float* w, int n, int pos_dim, int val_dim, float* out,
                      void* stream);
/* gather_backwards_with_precomputation (LatticeGPU.cuh:3761-3817); grad_values zeroed by caller. */
int ln_gather_backward(const float* grad_gathered, const int* idx, const float* w, int n, int pos_dim, int val_dim,
                       float* grad_values, void* stream);

/* slice_classify_with_precomputation (LatticeGPU.cuh:3387-3464): logits[n, C] (fully written). */
int ln_slice_classify_forward(const float* values, const float* delta_w, const float* lin_w, const float* lin_b,
                              const int* idx, const float* w, int n, int pos_dim, int val_dim, int nr_classes,
                              float* logits, void* stream);
/* slice_classify_backwards_with_precomputation (LatticeGPU.cuh:3628-3756).  g_delta_w, g_lin_w, g_lin_b are
 * caller-allocated, zeroed (lattice_funcs.py:554-557) and accumulated into.  The gradient wrt the lattice values
 * is a scatter of grad_sliced[n, V] (= dL/d sliced features, written here) with weights w_eff[n*(d+1)] (= w +
 * delta_w, written here): pass g_values = NULL and run ln_csr_reduce_rows(csr, grp_row, .., grad_sliced, w_eff, V,
 * d+1, V, g_values) on the adjacency of `idx` (no atomics), or pass g_values (zeroed [M, V]) to have it scattered
 * here with global atomics.  workspace: ln_slice_classify_backward_workspace_bytes. */
size_t ln_slice_classify_backward_workspace_bytes(int n, int pos_dim, int val_dim, int nr_classes);
int ln_slice_classify_backward(const float* grad_logits, const float* values, const float* delta_w, const float* lin_w,
                               const int* idx, const float* w, int n, int pos_dim, int val_dim, int nr_classes,
                               float* g_values, float* g_delta_w, float* g_lin_w, float* g_lin_b, float* grad_sliced,
                               float* w_eff, void* workspace, size_t workspace_bytes, void* stream);

/* Both gradients of out = ln_conv_forward(nbr_q, values_neigh, filter[E*val_dim, nr_filters]) in one call:
 * grad_filter as ln_conv_grad_filter(nbr_q, values_neigh, grad_out, mq, ..), grad_values[mn, val_dim] as
 * ln_conv_forward(nbr_n, grad_out, filter, mn, E, nr_filters, val_dim, FLIP | TRANSPOSED_FILTER) where nbr_n is the
 * neighbour list with the query / neighbour roles swapped.  For the small-filter shapes the slab sum of the filter
 * gradient runs inside the value-gradient launch.  workspace: ln_conv_backward_workspace_bytes (with less, down to
 * ln_conv_grad_filter_workspace_bytes(mq, ..), the value-gradient convolution runs without bank or slot split).  `row_partition` (may be
 * NULL) as for ln_conv_forward_ws: the table of the rows when both sides are the same lattice. */
size_t ln_conv_backward_workspace_bytes(int mq, int mn, int filter_extent, int val_dim, int nr_filters);
int ln_conv_backward(const int* nbr_q, const int* nbr_n, const float* values_neigh, const float* grad_out, const float* filter, int mq, int mn,
                     int filter_extent, int val_dim, int nr_filters, float* grad_values, float* grad_filter, void* workspace,
                     size_t workspace_bytes, const int* row_partition, void* stream);
/* ln_conv_backward with `flags`: 0 or LN_CONV_OVERLAPPED (the value gradient is the same bit for bit; the filter gradient is summed
 * over other row groups, so it differs in rounding only).  Same workspace size. */
int ln_conv_backward_flags(const int* nbr_q, const int* nbr_n, const float* values_neigh, const float* grad_out, const float* filter, int mq,
                           int mn, int filter_extent, int val_dim, int nr_filters, int flags, float* grad_values, float* grad_filter,
                           void* workspace, size_t workspace_bytes, const int* row_partition, void* stream);

/* Half-precision feature path of the scatters and the slice (C5: "features fp16, accumulate fp32"): the segment reduce with
 * fp16 source rows (fp32 weights, fp32 accumulation into an fp32 dst) — plain and fused with the neighbour traversal — and the
 * slice of fp16 lattice values into fp16 rows (fp32 arithmetic, val_dim % 4 == 0). */
int ln_csr_reduce_rows_f16(const LnCsr* csr, const int* grp_row, long long max_segments, const void* src_f16, const float* w, int val_dim,
                           int src_div, int src_stride, float* dst, void* stream);
int ln_splat_accumulate_and_neighbours_f16(const LnCsr* csr, const int* grp_row, long long max_segments, const void* src_f16, const float* w,
                                           int val_dim, int src_div, int src_stride, float* dst, const LnTable* table, int query_rows_upper,
                                           int* nbr, void* stream);
int ln_slice_forward_f16(const void* values_f16, const int* idx, const float* w, int n, int pos_dim, int val_dim, void* out_f16, void* stream);
/* ... that also zero-fills the fp32 accumulator of this slice's backward pass (as ln_slice_forward_prepare_backward). */
int ln_slice_forward_f16_prepare_backward(const void* values_f16, const int* idx, const float* w, int n, int pos_dim, int val_dim, void* out_f16,
                                          float* grad_accumulator, long long grad_accumulator_elems, void* stream);

/* DeformSlice head on fp16 lattice values (csrc/ln_classify_f16.hip).  `values_f16` is IEEE fp16 (`_Float16`) [M, val_dim], widened on
 * load; every other operand, every output and every accumulator is fp32.  Each call gives, bit for bit, what its fp32 namesake gives
 * on the same values widened to fp32 (same tiles, grids, slab layout and order of operations).
 *
 * ln_gather_forward_f16: out[n, (d+1)(V+1)] fp32, fully written, laid out as by ln_gather_forward.  Any val_dim >= 1, no alignment
 * asked for.  (The gather backward stays ln_gather_backward / the fp32 segment reduce of the fp32 grad_gathered.) */
int ln_gather_forward_f16(const void* values_f16, const int* idx, const float* w, int n, int pos_dim, int val_dim, float* out, void* stream);
/* ln_slice_classify_forward_f16: arguments of ln_slice_classify_forward.  Covers exactly the shapes at which that call takes its
 * wave-tiled form (val_dim % 32 == 0, nr_classes <= 32, nr_classes * val_dim <= 4096, pos_dim in {2, 3}) or a 4-channel form
 * (val_dim % 4 == 0 and a tile of 64 / 32 / 16 points within 64 KiB of LDS), with `values_f16` 8-byte aligned.  Any other shape
 * (val_dim % 4 != 0 among them) and a misaligned `values_f16` are LN_ERR_UNSUPPORTED, the message names V, C and d, nothing is
 * written.  n == 0 returns LN_OK. */
int ln_slice_classify_forward_f16(const void* values_f16, const float* delta_w, const float* lin_w, const float* lin_b, const int* idx,
                                  const float* w, int n, int pos_dim, int val_dim, int nr_classes, float* logits, void* stream);
/* ln_slice_classify_backward_f16: arguments and accumulate-into semantics of ln_slice_classify_backward (g_delta_w, g_lin_w, g_lin_b are
 * added to; grad_sliced[n, V] and w_eff[n (d+1)] are written), all fp32.  `g_values` must be NULL (LN_ERR_ARG): the value gradient is the
 * segment reduce of grad_sliced with w_eff (ln_csr_reduce_rows into an fp32 [M, V] buffer).  Covers exactly the shapes at which the fp32
 * call takes its wave-tiled form (val_dim % 32 == 0, val_dim <= 128, nr_classes <= 32, pos_dim in {2, 3}) or its 4-channel form
 * (val_dim % 4 == 0, 4 ceil(C / 4) * val_dim <= 12288, a tile of 64 .. 8 points within 64 KiB of LDS), with `values_f16` 8-byte and
 * grad_sliced 16-byte aligned; any other shape or alignment is LN_ERR_UNSUPPORTED (V, C and d named, nothing written), a workspace below
 * ln_slice_classify_backward_f16_workspace_bytes LN_ERR_WORKSPACE.  The workspace size is that of the fp32 call. */
size_t ln_slice_classify_backward_f16_workspace_bytes(int n, int pos_dim, int val_dim, int nr_classes);
int ln_slice_classify_backward_f16(const float* grad_logits, const void* values_f16, const float* delta_w, const float* lin_w,
                                   const int* idx, const float* w, int n, int pos_dim, int val_dim, int nr_classes, float* g_values,
                                   float* g_delta_w, float* g_lin_w, float* g_lin_b, float* grad_sliced, float* w_eff, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* Half-precision feature path of the convolution (BASELINE.json config 5 / SURVEY.md 8d C5: features fp16, accumulate
 * fp32).  Same arguments and flags as ln_conv_forward / ln_conv_grad_filter; values, filter bank, grad_out and out are
 * IEEE fp16 (`_Float16`), accumulation is fp32 (v_mfma_f32_16x16x16_f16 for val_dim in {16,32,64,96,128,256} and
 * nr_filters % 16 == 0; any other shape on a scalar kernel), the filter gradient is returned in fp32. */
int ln_conv_forward_f16(const int* nbr, const void* values_neigh, const void* filter, int m, int filter_extent, int val_dim,
                        int nr_filters, int flags, void* out, void* stream);
size_t ln_conv_grad_filter_f16_workspace_bytes(int m, int filter_extent, int val_dim, int nr_filters);
int ln_conv_grad_filter_f16(const int* nbr, const void* values_neigh, const void* grad_out, int m, int filter_extent, int val_dim,
                            int nr_filters, float* grad_filter, void* workspace, size_t workspace_bytes, void* stream);

/* "Next" row: the per-token MLP of PointNetModule (lattice_modules.py:636-676) on the distributed rows —
 * y[rows, cout] = act(x[rows, cin] @ w[cout, cin]^T + b), act = LeakyReLU(slope) (slope < 0: identity).  Streaming
 * kernels for rows ~ 10^5..10^6 and cin, cout <= 128, where a BLAS GEMM with K = 4..32 is far off the memory roofline
 * (float4 lanes when the channel count is a multiple of 4, scalar lanes otherwise).  backward: grad_x may be NULL (inputs
 * that need no gradient), grad_b may be NULL; `y` is the forward output (the activation mask is its sign);
 * cin * cout <= 10240. */
int ln_linear_act_forward(const float* x, const float* w, const float* b, long long rows, int cin, int cout, float slope, float* y,
                          void* stream);
size_t ln_linear_act_backward_workspace_bytes(int cin, int cout);
int ln_linear_act_backward(const float* x, const float* w, const float* y, const float* grad_y, long long rows, int cin, int cout,
                           float slope, float* grad_x, float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, void* stream);

/* "Next" row: GroupNorm (+ optional fused ReLU) of the LNN blocks on the native [m, channels]
 * value layout (lattice_modules.py:585-616 runs torch.nn.GroupNorm on a transposed [1, C, M] view).  Statistics
 * per group over (all rows) x (channels of the group), biased variance, as torch.nn.GroupNorm.
 * forward:  y = act(x * a[c] + b[c]),  a = gamma*rstd[g], b = beta - mean[g]*a;  also writes mean_rstd[2*groups]
 *           (means then rstds) and scale_shift[2*channels] (a then b) for the backward pass.
 * backward: grad_x (and grad_gamma / grad_beta when non-NULL) from x, grad_y and the two saved vectors.
 * channels % 4 == 0, channels <= 1024, 16-byte aligned tensors; workspace = ln_group_norm_workspace_bytes(channels).
 * next_workspace (may be NULL): a caller that alternates two workspaces on one stream passes the other one here; the
 * call then trusts `workspace` to be all-zero (no fill launch) and zero-fills next_workspace_bytes of `next_workspace` (what
 * its last user dirtied) before it returns the GPU. */
size_t ln_group_norm_workspace_bytes(int channels);
int ln_group_norm_forward(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps, int relu,
                          float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes, void* next_workspace,
                          size_t next_workspace_bytes, void* stream);
int ln_group_norm_backward(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd, const float* scale_shift, int m,
                           int channels, int groups, int relu, float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                           size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, void* stream);
/* The same with a device-side row count (static-rows mode: the [m, channels] tensors are taller than the lattice they hold):
 * rows_device == NULL, or one device int — the statistics run over min(m, *rows_device) rows, rows beyond are written as zeros
 * (y, grad_x) and contribute to nothing.  Pass LnTable.nr_filled of the lattice the values belong to. */
int ln_group_norm_forward_rows(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps, int relu,
                               float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes, void* next_workspace,
                               size_t next_workspace_bytes, const int* rows_device, void* stream);
int ln_group_norm_backward_rows(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd, const float* scale_shift, int m,
                                int channels, int groups, int relu, float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                                size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, const int* rows_device, void* stream);

/* GroupNorm per cloud for a batch of clouds in one table (LnTable.batch_points).  In first-occurrence row order
 * (LN_BUILD_CANONICAL_ROWS) the vertices of cloud s are the rows [row_starts[s], row_starts[s + 1]) of the value matrix: the points
 * of a batch are cloud-major and clouds share no vertex.
 * ln_cloud_row_starts writes row_starts[clouds + 1] (int32; row_starts[clouds] = min(*t->nr_filled, rows_upper, t->row_limit if
 * set), a cloud without a vertex starts where the next one does) from the first key coordinate of every row, with no host readback,
 * and *order_flag = 1 when some row's cloud is smaller than its predecessor's (the rows are not cloud-major: row_starts is not
 * usable), 0 otherwise.  1 <= clouds <= 64 (LN_ERR_UNSUPPORTED; ln_cloud_row_starts_many: the same call, 1 <= clouds <= 1024); the clouds must keep within half of t->batch_key_step of the origin.
 * ln_group_norm_forward_segments / _backward_segments: ln_group_norm_forward_rows / _backward_rows over `segments` row ranges of one
 * matrix, each normalised with the statistics of its own rows: the same blocking of the rows, counted from the start of the range,
 * the same summation, accumulator slab s for range s.  mean_rstd [segments, 2 * groups], scale_shift [segments, 2 * channels];
 * grad_gamma / grad_beta are the sums over the ranges, added in fp64 in range order.  The rows that count end at min(m,
 * row_starts[segments], *rows_device when given); the rows from there to m are written as zeros (y, grad_x).  An empty range writes
 * nothing (its mean_rstd / scale_shift rows keep their contents) and adds nothing.  Limits and the next_workspace alternation as for
 * ln_group_norm_forward; 1 <= segments <= 64; workspace = ln_group_norm_segments_workspace_bytes(channels, segments): `segments`
 * accumulator slabs of ln_group_norm_workspace_bytes(channels), then segments x 2 channels doubles the backward call keeps its
 * per-range parameter-gradient terms in.
 * ln_group_norm_forward_many_segments / _backward_many_segments: the same calls for 1 <= segments <= 1024.  Up to 64 segments they are
 * the calls above, launch for launch.  Beyond, a form made for many short ranges: one workgroup owns one range, takes its sums in LDS in
 * a fixed order (no accumulator slab, no atomic: two runs give the same bits) and writes its rows in the same launch; a long range is
 * correct and slow, one workgroup walks it.  There ln_group_norm_segments_workspace_bytes(channels, segments) is segments x 2 channels
 * doubles, the parameter-gradient terms of the backward call, none of which has to be zero on entry. */
int ln_cloud_row_starts(const LnTable* t, int rows_upper, int clouds, int* row_starts, int* order_flag, void* stream);
int ln_cloud_row_starts_many(const LnTable* t, int rows_upper, int clouds, int* row_starts, int* order_flag, void* stream);
size_t ln_group_norm_segments_workspace_bytes(int channels, int segments);
int ln_group_norm_forward_segments(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps, int relu,
                                   float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes, void* next_workspace,
                                   size_t next_workspace_bytes, const int* rows_device, const int* row_starts, int segments, void* stream);
int ln_group_norm_backward_segments(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd, const float* scale_shift,
                                    int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                                    size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, const int* rows_device,
                                    const int* row_starts, int segments, void* stream);
int ln_group_norm_forward_many_segments(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                        int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                        void* next_workspace, size_t next_workspace_bytes, const int* rows_device, const int* row_starts,
                                        int segments, void* stream);
int ln_group_norm_backward_many_segments(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                         const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                         float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                         size_t next_workspace_bytes, const int* rows_device, const int* row_starts, int segments, void* stream);

/* GroupNorm per row range on fp16 matrices: ln_group_norm_forward_segments / _backward_segments argument for argument, with x, y,
 * grad_y and grad_x pointing at IEEE half-precision elements ([m, channels], row-major).  An element is converted to fp32 as it is read
 * (exact) and rounded to nearest-even once as it is written; everything in between — the assignment of rows to threads, the fp32 / fp64
 * sums and their order, the statistics, the grids — is that of the fp32 call on the same numbers, so mean_rstd, scale_shift, grad_gamma
 * and grad_beta are those of the fp32 call on the converted inputs bit for bit, and y / grad_x are its outputs rounded to fp16.  The
 * ReLU mask of the backward call is x * a + b > 0 in fp32, not y > 0 of the rounded output.  gamma, beta, mean_rstd, scale_shift,
 * grad_gamma, grad_beta and the workspace (ln_group_norm_segments_workspace_bytes) are what they are in the fp32 calls.  The matrices
 * must be 8-byte aligned (LN_ERR_ARG); 1 <= segments <= 64 (there is no fp16 form of the _many_segments calls, nor of the calls over
 * the whole matrix: one range is the whole matrix); every other limit and error code is that of the fp32 call.  A refused call launches
 * and writes nothing. */
int ln_group_norm_forward_segments_f16(const void* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps, int relu,
                                       void* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                       void* next_workspace, size_t next_workspace_bytes, const int* rows_device, const int* row_starts,
                                       int segments, void* stream);
int ln_group_norm_backward_segments_f16(const void* x, const void* grad_y, const float* gamma, const float* mean_rstd, const float* scale_shift,
                                        int m, int channels, int groups, int relu, void* grad_x, float* grad_gamma, float* grad_beta,
                                        void* workspace, size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes,
                                        const int* rows_device, const int* row_starts, int segments, void* stream);

/* BatchNorm (+ optional fused ReLU) of BatchNormLatticeModule / BnReluConv (lattice_modules.py:570-583, 988-1009: torch.nn.BatchNorm1d
 * on the [m, channels] values), with the device-side row count of the _rows calls above: n = min(m, *rows_device) rows count (n = m
 * when rows_device is NULL), rows beyond n are written as zeros (y, grad_x) and contribute to nothing.
 * training != 0: statistics per channel over the n live rows (GroupNorm with one channel per group: the same sums, biased variance
 *           clamped at 0);  y = act(x * a[c] + b[c]),  a = gamma * rstd[c],  b = beta - mean[c] * a;  writes mean_rstd[2 * channels]
 *           (batch means then rstds) and scale_shift[2 * channels] (a then b) for the backward call, and moves the running statistics
 *           in place, with no host readback:  running_mean = (1 - momentum) running_mean + momentum mean,  running_var = (1 - momentum)
 *           running_var + momentum var n / (n - 1)  (unbiased, as torch), each formed in fp64 and rounded to fp32 once.
 *           n < 2: the running statistics keep their bits; the single live row has variance 0 and rstd = 1 / sqrt(eps), i.e. y =
 *           act(beta) up to rounding; n = 0 writes only zeros.  running_mean == running_var == NULL (track_running_stats=False):
 *           nothing is updated.
 * training == 0: the running statistics ARE the statistics (both required, LN_ERR_ARG otherwise) and are never written, by the forward
 *           or by the backward call:  a = gamma / sqrt(running_var + eps),  b = beta - running_mean * a  (rstd and b formed in fp64 and
 *           rounded once); mean_rstd holds (running means, rstds).  One launch, no sums; `workspace` is not touched (it may be NULL) by
 *           the forward call.  The backward call always needs the workspace, in either mode (its sums for grad_gamma / grad_beta).
 * backward: training: grad_x = gy' gamma rstd + x c2 + c3,  grad_gamma = (ds - db mean) rstd,  grad_beta = db  (the GroupNorm formula
 *           at groups == channels);  evaluation: grad_x = gy' a, grad_gamma / grad_beta the same expressions with the running mean.
 *           gy' = grad_y masked by fl(fl(x a) + b) > 0 with ReLU.  `training` must be what the forward call was given.
 * gamma, beta, running_mean, running_var, grad_gamma, grad_beta and rows_device may be NULL.  Limits, workspace and the next_workspace
 * alternation as for GroupNorm: float32, channels % 4 == 0, channels <= 1024 (LN_ERR_UNSUPPORTED), m >= 1, x / y / grad tensors 16-byte
 * aligned (LN_ERR_ARG); a rejected call launches nothing. */
size_t ln_batch_norm_workspace_bytes(int channels);
int ln_batch_norm_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, int m, int channels,
                          float eps, double momentum, int training, int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace,
                          size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, const int* rows_device, void* stream);
int ln_batch_norm_backward(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd, const float* scale_shift, int m,
                           int channels, int training, int relu, float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                           size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, const int* rows_device, void* stream);

/* ---- max-centring of the gathered simplex rows in the DeformSlice head ------------------------------------------
 * Replaces the torch broadcasting at lattice_modules.py:525-529 (`rowified -= gamma * max_vals + beta`, max over the
 * d+1 vertices of a simplex) and its autograd backward, whose two reductions over the N points dominate it.
 * x, out, grad_out, grad_x: [n, k, c] (k = d+1 <= 8 vertex rows of c <= 64 values per point); gamma, beta: [c].
 * Forward also emits max_vals [n, c] and arg_max [n, c] (u8, first maximum) for the backward pass.
 * Backward: grad_x = grad_out - [k == arg_max] * gamma * sum_k grad_out;  grad_gamma_beta [2, c]: row 0 =
 * -sum_n s*max, row 1 = -sum_n s with s = sum_k grad_out (summed in a fixed order: deterministic). */
int ln_max_centre_forward(const float* x, const float* gamma, const float* beta, long long n, int k, int c, float* out,
                          float* max_vals, unsigned char* arg_max, void* stream);
size_t ln_max_centre_backward_workspace_bytes(long long n, int k, int c);
int ln_max_centre_backward(const float* grad_out, const float* max_vals, const unsigned char* arg_max, const float* gamma,
                           long long n, int k, int c, float* grad_x, float* grad_gamma_beta, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Both gradients of a per-row linear layer y = x w^T (x [rows, cin], w [cout, cin]: the 1 x 1 layers of the blocks, run as lattice
 * convolutions over the identity neighbour list `ident` [rows, 1] = 0 .. rows-1): grad_w [cout, cin] and grad_x [rows, cin] (may be
 * NULL).  One call so that the slab sum of the weight gradient rides in the bank split of the input gradient's convolution. */
size_t ln_linear_backward_workspace_bytes(int rows, int cin, int cout);
int ln_linear_backward(const int* ident, const float* x, const float* grad_y, const float* w, int rows, int cin, int cout, float* grad_x,
                       float* grad_w, void* workspace, size_t workspace_bytes, void* stream);

/* The per-row linear layer on fp16 rows (the 1 x 1 layers on the half-precision feature path): a dense GEMM, no neighbour list.
 * x [rows, cin], y / residual [rows, cout], grad_y [rows, cout], grad_x [rows, cin]: IEEE fp16 (`_Float16`), contiguous;
 * w [cout, cin], bias [cout], grad_w [cout, cin], grad_b [cout]: fp32 (the master weights of the other fp16 operators).
 *   y[r, o]      = fp16( sum_k x[r, k] h(w[o, k]) + bias[o] + residual[r, o] )    bias, residual: optional (NULL)
 *   grad_x[r, k] = fp16( sum_o grad_y[r, o] h(w[o, k]) )                          optional (NULL: w is not read)
 *   grad_w[o, k] = sum_r grad_y[r, o] x[r, k]        grad_b[o] = sum_r grad_y[r, o]   (grad_b optional)
 * h rounds a weight to fp16 (to nearest-even) once, when a workgroup stages its bank; products are exact in fp32, every sum is
 * accumulated in fp32, bias and residual are added in fp32 and the result is rounded ONCE on store, as a conversion rounds: beyond
 * the fp16 range to +-inf, no clamping.  The gradient with respect to the residual is grad_y itself.  The row sums of grad_w and
 * grad_b go through one fp32 slab per 512 rows in `workspace` and are summed in slab order: no float atomics, every output bitwise
 * the same run to run.  A row never meets another row's values (a NaN in one row of x stays in that row of y), and rows from `rows`
 * on are never read.
 * Forms (csrc/ln_linear_f16_plan.h): cin and cout multiples of 16 up to 256 with x / w / residual / y (grad_y / w / grad_x; x / grad_y)
 * 8-byte aligned run on v_mfma_f32_16x16x32_f16 (the 16x16x16 form where the contraction length is no multiple of 32); any other
 * shape or alignment on one thread per output element, the weight gradient on one thread per (o, k) pair of a chunk.
 * rows == 0 is legal: nothing is read, grad_w and grad_b are written as zeros, the workspace is neither needed nor touched.
 * Refused, with nothing launched and nothing written: rows < 0, cin < 1, cout < 1, a null x / w / y (forward, rows > 0), a null
 * grad_w, a null x / grad_y (rows > 0), a null w with grad_x wanted (LN_ERR_ARG); a workspace that is null or smaller than
 * ln_linear_backward_f16_workspace_bytes(rows, cin, cout) at rows > 0 (LN_ERR_WORKSPACE); more output elements or (o, k) pairs
 * than one launch of the element-wise forms reaches (LN_ERR_UNSUPPORTED). */
int ln_linear_forward_f16(const void* x_f16, const float* w, const float* bias, const void* residual_f16, int rows, int cin, int cout,
                          void* y_f16, void* stream);
size_t ln_linear_backward_f16_workspace_bytes(int rows, int cin, int cout);
int ln_linear_backward_f16(const void* x_f16, const void* grad_y_f16, const float* w, int rows, int cin, int cout, void* grad_x_f16,
                           float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, void* stream);

/* ---- launch diet of the glue around the lattice operators in a training step ----------------------------------------------
 * Weight normalisation of the reference's weight_norm_wrapper with v_dim=None (latticenet_py/lattice/utils.py:72-158; LinearWN,
 * ConvLatticeIm2RowWN, CoarsenLatticeWN, FinefyLatticeWN):  w = v * g / ||v||_F  for v [rows, cols] and one magnitude per row
 * (g_dim 0, g [rows]) or per column (g_dim 1, g [cols]); at most 1024 magnitudes, rows * cols <= 2^24 (LN_ERR_UNSUPPORTED);
 * rows, cols >= 1, g_dim 0 or 1, no null buffer (LN_ERR_ARG); a rejected call launches nothing.  One workgroup each way,
 * sums in a fixed order.  `norm`: one float written by the forward call and read by the backward call.
 *   grad_g[j] = sum_k grad_w[j,k] v[j,k] / n      grad_v = grad_w * g / n - v * (sum_j g[j] sum_k grad_w[j,k] v[j,k]) / n^3 */
int ln_weight_norm_forward(const float* v, const float* g, int rows, int cols, int g_dim, float* w, float* norm, void* stream);
int ln_weight_norm_backward(const float* v, const float* g, const float* grad_w, const float* norm, int rows, int cols, int g_dim,
                            float* grad_v, float* grad_g, void* stream);

/* DistributeLatticeModule's per-token tail (lattice_modules.py:72-94) in one pass: distributed / out [tokens, width] rows whose
 * first pos_dim columns are positions; position_sums [m, pos_dim] and counts [m] per vertex (ln_csr_reduce_rows of the positions
 * with unit weights, ln_csr_group_sizes);  out[t, :pos_dim] = d[t, :pos_dim] - sums[idx[t]] / max(counts[idx[t]], 1), the other
 * columns copied; rows of tokens with idx[t] <= 0 (no vertex, or vertex 0 = the "invalid" bucket) are zero. */
int ln_distribute_centre(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts, long long tokens,
                         int width, int pos_dim, float* out, void* stream);
/* The same for a batch of clouds in one table (LnTable.batch_points), where the reference's "invalid" vertex is the first vertex of
 * EVERY cloud, not row 0 of the table.  row_starts: device int32 [clouds + 1], what ln_cloud_row_starts writes; 1 <= clouds <= 64
 * (LN_ERR_UNSUPPORTED, nothing launched; ln_distribute_centre_many_clouds / _many_cloud_starts: the same calls, 1 <= clouds <= 1024).  Token t belongs to cloud min(t / tokens_per_cloud, clouds - 1), tokens_per_cloud =
 * LnTable.batch_points x (lattice pos_dim + 1) >= 1; its row is zero when idx[t] < 0 or idx[t] == row_starts[cloud of t], and gets the
 * arithmetic of ln_distribute_centre otherwise.  One cloud with row_starts[0] = 0 is ln_distribute_centre.  No host readback, no
 * allocation: safe inside a stream capture. */
int ln_distribute_centre_clouds(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                long long tokens, int width, int pos_dim, long long tokens_per_cloud, const int* row_starts, int clouds,
                                float* out, void* stream);
/* ln_distribute_centre_clouds for clouds of unequal sizes (LnTableClouds.batch_point_starts): token t belongs to point t / tokens_per_point
 * (tokens_per_point = lattice pos_dim + 1 >= 1) and the point to cloud upper_bound(point_starts, point) - 1, point_starts device int32
 * [clouds + 1] as in LnTable.  Everything else, the refusals included, as above; point_starts == NULL is LN_ERR_ARG. */
int ln_distribute_centre_cloud_starts(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                      long long tokens, int width, int pos_dim, int tokens_per_point, const int* point_starts,
                                      const int* row_starts, int clouds, float* out, void* stream);
int ln_distribute_centre_many_clouds(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                     long long tokens, int width, int pos_dim, long long tokens_per_cloud, const int* row_starts, int clouds,
                                     float* out, void* stream);
int ln_distribute_centre_many_cloud_starts(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                           long long tokens, int width, int pos_dim, int tokens_per_point, const int* point_starts,
                                           const int* row_starts, int clouds, float* out, void* stream);

/* The vertex-side reduction of PointNetModule (lattice_modules.py:688-712: scatter_max, scatter_add of ones, index_select of the
 * winning tokens' barycentric weights, cat, masked_fill(nr_points < 4), keep mask of vertex 0) over the token adjacency `csr`:
 *   out [rows, 2 * channels] = [max over the row's tokens of src[t, :] | bary[argmax token * bary_stride]]
 *   out_arg [rows, channels] = winning token, -1 where the row is dropped (fewer than min_points tokens, row 0) or has no token.
 * Backward wrt src, token-major (every element of grad_src [tokens, channels] is written: no fill, no scatter):
 *   grad_src[t, c] = grad_out[idx[t] * grad_stride + c] if out_arg[idx[t], c] == t else 0. */
size_t ln_pointnet_reduce_workspace_bytes(int rows, int channels);
int ln_pointnet_reduce_forward(const LnCsr* csr, const int* grp_row, long long max_segments, const float* src, int channels,
                               const float* bary, int bary_stride, int rows, int min_points, void* workspace, size_t workspace_bytes,
                               float* out, int* out_arg, void* stream);
/* ln_pointnet_reduce_forward for a batch of clouds in one table: the same segment max, counts, min_points rule and workspace, but the
 * decode step drops the invalid vertex of every cloud instead of row 0.  row_starts: device int32 [clouds + 1] (ln_cloud_row_starts),
 * 1 <= clouds <= 64 (LN_ERR_UNSUPPORTED, nothing launched).  ln_pointnet_reduce_forward_many_clouds: the same call for 1 <= clouds <=
 * 1024; beyond 64 clouds a second instance of the decode kernel holds up to 1025 starts in LDS and finds the cloud of a row by binary
 * search.  Row r is the invalid vertex of cloud c exactly when r == row_starts[c] and
 * row_starts[c] < row_starts[c + 1]: a cloud without a vertex has none, row_starts[clouds] is none; a dropped row gets out = 0 and
 * out_arg = -1.  No host readback, no allocation: safe inside a stream capture.
 * ln_pointnet_reduce_backward serves both: it selects by out_arg[idx[t], c] == t, and out_arg is -1 on every dropped row, so the tokens
 * of every cloud's invalid vertex get a zero gradient without a row_starts argument.  (It also skips the tokens of row 0 outright: with
 * row_starts[0] == 0, as ln_cloud_row_starts writes it, row 0 is the invalid vertex of the first cloud that has a vertex.) */
int ln_pointnet_reduce_forward_clouds(const LnCsr* csr, const int* grp_row, long long max_segments, const float* src, int channels,
                                      const float* bary, int bary_stride, int rows, int min_points, void* workspace, size_t workspace_bytes,
                                      float* out, int* out_arg, const int* row_starts, int clouds, void* stream);
int ln_pointnet_reduce_forward_many_clouds(const LnCsr* csr, const int* grp_row, long long max_segments, const float* src, int channels,
                                           const float* bary, int bary_stride, int rows, int min_points, void* workspace,
                                           size_t workspace_bytes, float* out, int* out_arg, const int* row_starts, int clouds, void* stream);
int ln_pointnet_reduce_backward(const float* grad_out, int grad_stride, const int* out_arg, const int* splat_idx, long long tokens,
                                int channels, float* grad_src, void* stream);

/* Mean negative log-likelihood of the training loop (ln_train.py:130, torch.nn.NLLLoss(ignore_index=...)): log_probs [n, classes]
 * float, target [n] int64; ignore_index: a label value that is skipped (pass a value no label takes, e.g. LLONG_MIN, for none).
 * loss_count [2]: {loss = -sum lp[i, y_i] / max(count, 1), max(count, 1)} (count = labels not ignored); labels outside
 * [0, classes) are clamped, as in the gather formulation it replaces.  Backward writes every element of grad_log_probs [n, classes]:
 * -grad_loss / count at (i, y_i) of the labels that count, 0 elsewhere.  Sums in a fixed order (deterministic).
 * This is the case of ONE cloud without class weights of ln_nll_forward_clouds / ln_nll_backward_clouds below, run by the same kernels
 * (csrc/ln_nll.hip): loss_count[0] is that call's per_cloud[0], loss_count[1] its weight_sum[0], and no mean over the clouds is taken
 * (one launch forward up to 1024 rows, two above; one backward).
 * n >= 0 (n == 0: loss 0, count 1; the backward writes nothing), classes >= 1, no null buffer, a workspace of at least
 * ln_nll_workspace_bytes() (all LN_ERR_ARG); n >= 2^31 or n * classes >= 2^31 (LN_ERR_UNSUPPORTED: the kernels index with 32 bits,
 * as every other loss entry point does); a rejected call launches nothing. */
size_t ln_nll_workspace_bytes(void);
int ln_nll_forward(const float* log_probs, const long long* target, long long n, int classes, long long ignore_index, void* workspace,
                   size_t workspace_bytes, float* loss_count, void* stream);
int ln_nll_backward(const long long* target, const float* grad_loss, const float* loss_count, long long n, int classes,
                    long long ignore_index, float* grad_log_probs, void* stream);

/* Lovasz-Softmax loss of the training loop (ln_train.py:156-158, lovasz_loss.py:17-57) over log_probs [n, classes] float and target
 * [n] int64 (labels outside [0, classes) are clamped), for all classes at once.  Per class c: p = exp(log_probs[:, c]),
 * fg_i = [label_i == c], e_i = |fg_i - p_i|; the errors in descending order, EQUAL ERRORS BY ASCENDING POINT INDEX (a stable sort);
 * loss_c = sum_k e_(k) g_k with the Jaccard gradient in closed form — G = #fg, U = G + #background and I = G - #foreground among
 * the first k+1 elements: g_k = 1 / U (element k foreground), I / (U (U - 1)) (background).  A class counts when G > 0 and
 * c != ignore_index (pass a value no class takes, e.g. LLONG_MIN, for none; points that carry the ignore label still act as
 * background of the other classes).  reduction 0: loss[0] = sum over the counting classes / max(#counting, 1); 1: the sum.
 * per_class [classes] (may be NULL): loss_c, 0 for a class that does not count.  p below the smallest normal float counts as 0.
 * The forward call also writes every element of dloss_dlogp [n, classes] = d loss / d log_probs = scale_c s g_rank(i) p_ic
 * (s = -1 foreground, +1 background; scale_c = 0 for a class that does not count, else 1 (sum) or 1 / #counting (mean));
 * ln_lovasz_backward multiplies it by grad_loss[0] into grad_log_probs [n, classes] (one elementwise launch).
 * Limits (LN_ERR_ARG otherwise, nothing launched): 1 <= classes <= 1024, n >= 0, n * classes < 2^31; n == 0 sets loss (and
 * per_class) to 0 and runs no sort.  All scratch is the caller's workspace (ln_lovasz_workspace_bytes: a pure host function);
 * no host synchronisation, no allocation: safe inside a stream capture.  Every sum is taken in a fixed order and there are no
 * float atomics: loss and gradient are bitwise reproducible. */
size_t ln_lovasz_workspace_bytes(long long n, int classes);
int ln_lovasz_forward(const float* log_probs, const long long* target, long long n, int classes, long long ignore_index, int reduction,
                      void* workspace, size_t workspace_bytes, float* loss, float* per_class, float* dloss_dlogp, void* stream);
int ln_lovasz_backward(const float* dloss_dlogp, const float* grad_loss, long long n, int classes, float* grad_log_probs, void* stream);

/* The same loss PER CLOUD for a batch of clouds in one matrix (Berman's per_image=True): the n rows are cloud-major, cloud b owns rows
 * [b n0, min((b + 1) n0, n)) with n0 = points_per_cloud, B = ceil(n / n0) clouds, the last one possibly shorter (what
 * Lattice.set_cloud_batch defines; points_per_cloud >= n is one cloud).  per_cloud [B] (may be NULL) and row b of per_class
 * [B, classes] (may be NULL) are what ln_lovasz_forward gives on cloud b's rows alone, bit for bit: the same arithmetic, ties by
 * ascending point index inside the cloud, the cloud's own set of counting classes; a cloud with no counting class has loss 0.
 * loss[0] = (sum_b per_cloud[b]) / B, the clouds added in a fixed order (strided over 256 threads in series, then the fixed tree of a
 * workgroup).  dloss_dlogp [n, classes], every element written: the single-cloud coefficient of the point within its cloud, divided
 * by B (one IEEE division: one more rounding, none when B is a power of two); a class that does not count in cloud b is 0 on that
 * cloud's rows only.
 * ln_lovasz_backward is the backward.  The sort works on B x classes segments of at most n0 items: keys, payloads and tile histograms
 * are per (cloud, class), a tile never spans two clouds, and the sort payload is the point's index INSIDE ITS CLOUD (plus the foreground
 * bit).  One launch more than ln_lovasz_forward (the mean over the clouds), none per cloud.
 * Limits (LN_ERR_ARG otherwise, nothing launched or written): points_per_cloud >= 1, n >= 0, 1 <= classes <= 1024, n * classes < 2^31,
 * B <= 65535 (the cloud is the z coordinate of the tile grids and the y coordinate of the scan grids, the class their y / x coordinate;
 * no grid has 2^32 work-items in one dimension: B x classes itself is bounded only by B <= 65535 and classes <= 1024), reduction 0 or 1,
 * a workspace of ln_lovasz_clouds_workspace_bytes (a pure host function, total).  The workspace grows with B x classes, not only with
 * n x classes: besides 16 bytes per (point, class) it holds 1 KB of digit histogram per (cloud, class, tile of 2048 points of a cloud),
 * however few points a cloud has — 700 clouds of 3 points at 20 classes take 14 MB, 65 535 clouds at 65 classes 4.4 GB.
 * n == 0 sets loss to 0 and runs no sort.  No host synchronisation, no allocation, no float atomics: safe inside a stream capture,
 * bitwise reproducible. */
size_t ln_lovasz_clouds_workspace_bytes(long long n, long long points_per_cloud, int classes);
int ln_lovasz_forward_clouds(const float* log_probs, const long long* target, long long n, long long points_per_cloud, int classes,
                             long long ignore_index, int reduction, void* workspace, size_t workspace_bytes, float* loss, float* per_cloud,
                             float* per_class, float* dloss_dlogp, void* stream);

/* Intersection / union counts of the validation metric (callbacks/scores.py), per cloud of such a batch, added onto the int64
 * accumulators intersection [classes] and union_ [classes].  scores [n, classes] float, target [n] int64.  Per cloud: pred_i = the
 * lowest class index among the maxima of row i (torch.argmax); hit_c = #{pred = target = c} with the UNCLAMPED label (a label outside
 * [0, classes) never hits); n_gt_c counts labels clamped to [0, classes - 1]; n_pred_c = #{pred = c}; in_gt_c = n_gt_c > 0 and
 * c != unlabeled_index (any value outside [0, classes) for none).  intersection[c] += sum_b hit in_gt, union_[c] += sum_b (n_gt +
 * n_pred - hit) in_gt — Scores.accumulate_scores called cloud by cloud.  All integer: exact and independent of any order.  Rows that
 * hold a NaN are NOT held to torch's rule.  Limits and host behaviour as ln_lovasz_forward_clouds (the cloud is the y coordinate of
 * the grid: B <= 65535); n == 0 adds nothing. */
size_t ln_iou_counts_clouds_workspace_bytes(long long n, long long points_per_cloud, int classes);
int ln_iou_counts_clouds(const float* scores, const long long* target, long long n, long long points_per_cloud, int classes,
                         long long unlabeled_index, void* workspace, size_t workspace_bytes, long long* intersection, long long* union_,
                         void* stream);

/* Generalized soft Dice loss of the training loop (ln_train.py:127, diceloss.py:172-209) over log_probs [n, classes] float and target
 * [n] int64, one cloud or PER CLOUD of a cloud-major batch (clouds as ln_lovasz_forward_clouds defines them: cloud b owns rows
 * [b n0, min((b + 1) n0, n)) with n0 = points_per_cloud, B = ceil(n / n0), the last one possibly shorter; points_per_cloud >= n is one
 * cloud).  Per cloud, with p = exp(log_probs) and w_c = 0 for c == ignore_index (pass a value no class takes, e.g. LLONG_MIN, for none),
 * else 1:  I_c = sum_i p_ic [y_i = c], S_c = sum_i p_ic, G_c = #{y_i = c}, D_c = S_c + G_c + 1e-6, the cloud's loss =
 * sum_c w_c (1 - 2 I_c / D_c) / classes.  Points labelled ignore_index still count in S of every class, the division is by all
 * classes, a class absent from the cloud contributes w_c / classes.  A LABEL OUTSIDE [0, classes) BELONGS TO NO CLASS: its point
 * counts in S only (the torch form faults on such a label).
 * loss[0] = the mean over the clouds of each cloud's loss, the clouds added in a fixed order (strided over 256 threads in series, then
 * the fixed tree of a workgroup).  per_cloud [B] (may be NULL): the clouds' losses.  stats [B, 3, classes] (may be NULL): I, S and G as
 * float.  coef [B, 2, classes]: a_c = 2 w_c / (classes D_c) / B and b_c = a_c I_c / D_c, what the backward needs.  per_cloud[b] and
 * stats[b] are what the call gives on cloud b's rows alone, bit for bit: a cloud is cut into tiles by its own length.
 * ln_dice_backward (one elementwise launch) writes every element of grad_log_probs [n, classes]:
 * -grad_loss[0] p_ic (a_c [y_i = c] - b_c) with the coefficients of the point's cloud; the caller does not zero the buffer; an entry
 * with log_probs = -inf gets 0.  Called with the sizes of the forward call.
 * Limits (LN_ERR_ARG otherwise, nothing launched or written): points_per_cloud >= 1, n >= 0, 1 <= classes <= 1024, n * classes < 2^31,
 * B <= 65535 (the cloud is the y coordinate of the grid), no null buffer but the optional ones, a workspace of ln_dice_workspace_bytes
 * (a pure host function, total; at most 24 bytes per (point, class) and 16 per (cloud, class)).  n == 0: ln_dice_forward sets loss to 0,
 * ln_dice_backward launches nothing.  Two launches forward, one backward; no host synchronisation, no allocation, no float atomics:
 * safe inside a stream capture, bitwise reproducible.  Rows that hold a NaN are not held to any rule. */
size_t ln_dice_workspace_bytes(long long n, long long points_per_cloud, int classes);
int ln_dice_forward(const float* log_probs, const long long* target, long long n, long long points_per_cloud, int classes,
                    long long ignore_index, void* workspace, size_t workspace_bytes, float* loss, float* per_cloud, float* stats, float* coef,
                    void* stream);
int ln_dice_backward(const float* log_probs, const long long* target, const float* coef, const float* grad_loss, long long n,
                     long long points_per_cloud, int classes, float* grad_log_probs, void* stream);

/* Class-weighted mean negative log-likelihood PER CLOUD of a cloud-major batch: torch.nn.NLLLoss(weight=, ignore_index=) on every cloud
 * and the mean over the clouds (ln_train.py:130 on each cloud of a batch; weights as models.py compute_class_weights makes them).
 * log_probs [n, classes] float, target [n] int64; clouds as ln_dice_forward defines them: cloud b owns rows [b n0, min((b + 1) n0, n))
 * with n0 = points_per_cloud, B = ceil(n / n0), the last one possibly shorter; points_per_cloud >= n is one cloud.  A label counts when
 * it differs from ignore_index (pass a value no label takes, e.g. LLONG_MIN, for none); labels outside [0, classes) are clamped, as in
 * ln_nll_forward, and take the weight of the class they clamp to.  class_weight [classes] float or NULL (every weight 1).  Per cloud:
 * N_b = sum w[y_i] log_probs[i, y_i] and W_b = sum w[y_i] over the labels that count; weight_sum[b] = W_b, or 1 when W_b == 0 (no label
 * counts, or every counted weight is zero) — what the backward divides by —; per_cloud[b] = -N_b / weight_sum[b] (0 for such a cloud);
 * loss[0] = (sum_b per_cloud[b]) / B, the convention of ln_lovasz_forward_clouds and ln_dice_forward.  log_probs is read at the clamped
 * label of the rows that count and nowhere else, class_weight at the classes of such labels only: a -inf or NaN anywhere else reaches
 * no output.
 * Every sum in a fixed order, no float atomics.  The workgroups, strides, shuffle trees and finishing order of a cloud's sum depend on
 * the cloud's rows alone, so per_cloud[b] and weight_sum[b] are what this call gives on cloud b's rows alone, bit for bit; with
 * class_weight == NULL they are the loss_count of ln_nll_forward on those rows by construction: that entry point runs these kernels on
 * one cloud.  The clouds are added strided over 1024 threads in series, then by the fixed tree of that workgroup.
 * ln_nll_backward_clouds (one elementwise launch) writes every element of grad_log_probs [n, classes]:
 * -grad_loss[0] w[y_i] / (B weight_sum[b]) at (i, clamped y_i) of the labels that count, 0 elsewhere; the caller does not zero the
 * buffer.  Called with the sizes, ignore_index and class_weight of the forward call.
 * Refused, nothing launched or written: n < 0, classes < 1, points_per_cloud < 1, a null buffer (but class_weight), a workspace below
 * ln_nll_clouds_workspace_bytes (a pure host function, total) — LN_ERR_ARG; n * classes >= 2^31, B > 65535 (the cloud is the y
 * coordinate of the grid) — LN_ERR_UNSUPPORTED.  n == 0: the forward sets loss to 0, the backward launches nothing.  Two launches
 * forward (three for more than 64 clouds of more than 1024 rows each), one backward; no host synchronisation, no allocation: safe
 * inside a stream capture, bitwise reproducible.  Not held: more than 2^24 counted labels in one cloud without weights (the fp32 count
 * stops being exact). */
size_t ln_nll_clouds_workspace_bytes(long long n, long long points_per_cloud);
int ln_nll_forward_clouds(const float* log_probs, const long long* target, long long n, long long points_per_cloud, int classes,
                          long long ignore_index, const float* class_weight, void* workspace, size_t workspace_bytes, float* loss,
                          float* per_cloud, float* weight_sum, void* stream);
int ln_nll_backward_clouds(const long long* target, const float* grad_loss, const float* weight_sum, long long n, long long points_per_cloud,
                           int classes, long long ignore_index, const float* class_weight, float* grad_log_probs, void* stream);

/* The three per-cloud losses above for a batch of clouds of UNEQUAL sizes (Lattice.set_cloud_batch([l_0, l_1, ...])): each _ranges
 * entry point takes what its counterpart takes, with (point_starts, clouds, longest) in place of points_per_cloud.  point_starts is a device
 * list of clouds + 1 ints, the list an LnTableClouds keeps as batch_point_starts; cloud b owns rows [point_starts[b], point_starts[b + 1]).
 * CONTRACT ON THE LIST: ascending, point_starts[0] = 0, point_starts[clouds] = n, no cloud longer than `longest` (the host's copy of the
 * longest length: grids and workspace strides are sized by it, nothing is read back).  WHATEVER THE LIST HOLDS, THE KERNELS STAY INSIDE THE
 * n ROWS and inside the workspace: a cloud's range is clamped into [0, n] and its length to `longest`; a list that breaks the contract
 * gives values without meaning, never an access out of bounds.
 * Everything else is the equal-size form: the arithmetic and the order of every sum (a cloud is cut and summed by its own length alone, so
 * per_cloud[b] and the per-cloud side outputs are what the one-cloud call gives on the cloud's rows, bit for bit, and lengths
 * (n0, .., n0, rest) give the bits of the equal-size entry point), no float atomics, one launch backward, the launches forward, safe inside
 * a stream capture (the list is read by the kernels only: the same pointer must hold the same lengths at every replay).
 * An EMPTY cloud (point_starts[b] == point_starts[b + 1]) is a legal cloud and counts in the mean over the clouds: NLL per_cloud 0 (as -0)
 * and weight_sum 1; Lovasz 0 (per_class row 0); Dice (classes other than ignore_index) / classes, stats 0, its coef row without meaning (no
 * row reads it); no gradient row.  The backward kernels find a row's cloud by a binary search of the
 * list that steps over empty clouds.  n == 0 (every cloud empty): the forward calls write those values and the mean, the backward calls
 * launch nothing.
 * Refused with nothing launched or written, the message of ln_last_error_string naming the entry point: point_starts == NULL, clouds < 1,
 * longest < 0 or longest > n (LN_ERR_ARG); clouds > 65535 and the size limits of the counterpart (n * classes < 2^31, classes <= 1024), with
 * the counterpart's code (LN_ERR_UNSUPPORTED for the NLL entries, LN_ERR_ARG otherwise); null buffers and a workspace below the
 * *_ranges_workspace_bytes function — pure host functions of (n, clouds, longest[, classes]), total over any arguments.  The Lovasz
 * workspace holds clouds x classes x tiles(longest) histograms: it grows with one long cloud among many short ones.
 * ln_lovasz_forward_ranges has no backward of its own: ln_lovasz_backward is the backward.
 * ln_iou_counts_clouds has no such form yet, and losses.py does not call these entry points yet: its points_per_cloud= takes equal sizes. */
size_t ln_nll_ranges_workspace_bytes(long long n, int clouds, long long longest);
int ln_nll_forward_ranges(const float* log_probs, const long long* target, long long n, const int* point_starts, int clouds, long long longest,
                          int classes, long long ignore_index, const float* class_weight, void* workspace, size_t workspace_bytes, float* loss,
                          float* per_cloud, float* weight_sum, void* stream);
int ln_nll_backward_ranges(const long long* target, const float* grad_loss, const float* weight_sum, long long n, const int* point_starts,
                           int clouds, long long longest, int classes, long long ignore_index, const float* class_weight,
                           float* grad_log_probs, void* stream);
size_t ln_dice_ranges_workspace_bytes(long long n, int clouds, long long longest, int classes);
int ln_dice_forward_ranges(const float* log_probs, const long long* target, long long n, const int* point_starts, int clouds, long long longest,
                           int classes, long long ignore_index, void* workspace, size_t workspace_bytes, float* loss, float* per_cloud,
                           float* stats, float* coef, void* stream);
int ln_dice_backward_ranges(const float* log_probs, const long long* target, const float* coef, const float* grad_loss, long long n,
                            const int* point_starts, int clouds, long long longest, int classes, float* grad_log_probs, void* stream);
size_t ln_lovasz_ranges_workspace_bytes(long long n, int clouds, long long longest, int classes);
int ln_lovasz_forward_ranges(const float* log_probs, const long long* target, long long n, const int* point_starts, int clouds,
                             long long longest, int classes, long long ignore_index, int reduction, void* workspace, size_t workspace_bytes,
                             float* loss, float* per_cloud, float* per_class, float* dloss_dlogp, void* stream);

/* Band check of a batch of clouds in one table (LnTable.batch_points / batch_key_step): a launch sequence of its own, queued on `stream`
 * behind the build of `t` from the same positions and sigmas; the build kernels are not involved.  B = ceil(n / batch_points) clouds, or,
 * for a table that heads an LnTableClouds, its batch_clouds clouds with the point ranges of its batch_point_starts (every cloud reduces
 * its own range, clamped to [0, n]).
 * extents [B, 2] int32 receives, per cloud, the smallest and the largest FIRST key coordinate over the d + 1 simplex vertices of every
 * point of the cloud, before the cloud's shift (an empty cloud keeps (INT_MAX, INT_MIN)); integer atomics only: order-independent and
 * bitwise reproducible.  With half = batch_key_step >> 1, cloud c is inside its band when -half + guard <= lo_c and hi_c < half - guard;
 * an empty cloud is inside.  *first_bad receives the smallest offending cloud, INT_MAX when there is none.  On a violation
 * LN_STATUS_CLOUD_BAND is ORed into *t->status and, when t->host_counters is set, the report word of the build is stored again with the
 * bit in it (*t->nr_filled | *t->status << 32 | host_seq << 40: pass the LnTable the build was given).  For an LnTableClouds, the
 * report word is stored again as well when *t->status holds LN_STATUS_CLOUD_STARTS (ln_cloud_point_starts_check queued in front of this
 * call): both bits travel to the host the same way.  Three launches, no host synchronisation, no allocation: safe inside a stream capture.
 * Refused, nothing launched or written: a null table, buffer or sigmas, a table without a batch (batch_points == 0), n < 0, guard < 0,
 * guard >= half — LN_ERR_ARG; pos_dim outside 1..LN_MAX_POS_DIM, B > 65535 (the cloud is the y coordinate of the grid) —
 * LN_ERR_UNSUPPORTED.  n == 0 launches and writes nothing.
 *
 * guard, in key units of the level that is checked (the finest).  Write e for the elevated first coordinate of a point.
 *  - The d + 1 vertices of the simplex that holds the point differ by at most d in every coordinate and the point is a convex combination
 *    of them; with one unit for the fp32 rounding of e, every vertex key k of the point has |k - e| <= d + 1.
 *  - A 1-hop neighbour at dilation 1 (csrc/ln_neighbours.h) is key + 1 in every coordinate but one, key - d in that one (or the mirror
 *    image): its first coordinate is at most d away, dilation x d at a larger dilation.
 *  - Level L (sigmas x 2^L, built from the same positions) has e / 2^L, exactly, as its elevated coordinate, and key step and band are
 *    halved L times (batch_key_step is a multiple of 16 (d + 1): exact for L <= 3).  A level-L key unit is 2^L units of the finest
 *    level, so in those units a level-L vertex of the point lies within 2^L (d + 1) of e, i.e. within (1 + 2^L)(d + 1) of a finest-level
 *    vertex of the point, and its 1-hop neighbours within (1 + 2^L)(d + 1) + 2^L d.
 *  So guard >= (1 + 2^L)(d + 1) + 2^L d keeps the vertices of level L and their 1-hop neighbours inside the band, and the row decode of
 *  ln_cloud_row_starts right, whenever the finest level passes.  L = 3: 9 (d + 1) + 8 d = 17 d + 9 <= 16 (d + 1) for d <= 7.  The
 *  default of the Python layer, 16 (d + 1), therefore covers four lattice levels (L = 0..3) at dilation 1 for every supported pos_dim;
 *  larger dilations or more levels need (1 + 2^L)(d + 1) + dilation 2^L d. */
int ln_cloud_key_extents(const LnTable* t, const float* positions_raw, const float* sigmas_host, int n, int guard, int* extents,
                         int* first_bad, void* stream);
/* Verifies on the device what LnTableClouds.batch_point_starts promises about `starts` (device int32 [clouds + 1]) for n points: starts[0] == 0,
 * starts[clouds] == n, starts[c] <= starts[c + 1].  One launch of one workgroup; on a violation LN_STATUS_CLOUD_STARTS is ORed into
 * *status (device int32, the table's status word), else nothing is written.  No host synchronisation, no allocation: safe inside a
 * stream capture.  Refused, nothing launched or written: null starts or status, clouds < 1, n < 0 — LN_ERR_ARG. */
int ln_cloud_point_starts_check(const int* starts, int clouds, int n, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LATTICENET_HIP_H */
