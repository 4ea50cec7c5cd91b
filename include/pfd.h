/* pfd.h — C-ABI of libpfd_hip.so: MI355X-native D8 flow-accumulation hot path.
 *
 * This is the drop-in boundary for the path
 *     D8 raster -> downstream graph -> cell ordering -> accuflux / upstream_area,
 *     Strahler order, basins, HAND
 * of Deltares/pyflwdir (reference v0.5.12).  The reference has no FFI of its own: its seam
 * is "method on FlwdirRaster validates & flattens, then calls a free function on flat
 * C-contiguous numpy arrays" (reference pyflwdir/flwdir.py:567-602, pyflwdir/pyflwdir.py:
 * 770-801, :564-599, :1485-1511).  Each entry point below replaces one of those free
 * functions and cites it.  Plain C: opaque handle, plain pointers and sizes, int status.
 *
 * Conventions
 *   - Every function returns PFD_OK (0) or a negative PFD_E* code; pfd_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - Rasters are row-major (C order), linear cell index i = r*ncol + c.
 *   - `memspace` says where the caller's buffers live: PFD_HOST (the library stages them
 *     through HBM) or PFD_DEVICE (pointers into the HBM of the handle's GPU; nothing is
 *     copied).  Inputs are never modified; outputs are caller-allocated and fully written.
 *   - A handle owns all device state (normalised D8 codes, level structure, scratch) of one
 *     raster (or one row block of a raster in a multi-GPU job) on one GPU.  Handles are not
 *     thread-safe; use one per host thread / process.
 */
#ifndef PFD_H_
#define PFD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFD_ABI_VERSION 1

/* status codes */
#define PFD_OK 0
#define PFD_EINVAL (-1)      /* bad argument (shape, dtype code, NULL pointer, ...) */
#define PFD_ENODEVICE (-2)   /* no usable HIP device / device index out of range */
#define PFD_EHIP (-3)        /* a HIP runtime call failed (message has the HIP error) */
#define PFD_ENOMEM (-4)      /* device or host allocation failed */
#define PFD_EBADCODE (-5)    /* raster holds a value that is not a D8 code (core_d8._all) */
#define PFD_ENOPITS (-6)     /* raster has no pit: reference raises "no pits found" */
#define PFD_EUNSUPPORTED (-7)/* valid request outside what the HIP path implements */
#define PFD_ECOMM (-8)       /* RCCL call failed (multi-GPU) */

/* memory spaces */
#define PFD_HOST 0
#define PFD_DEVICE 1
/* Ordering of PFD_DEVICE arguments, the one rule: a call returns only after everything it wrote to the caller's device
 * buffers is complete in HBM (the sweeps wait for their handle's stream, the elementwise calls and the device helpers
 * for the null stream), and it reads its device inputs only while it runs.  So a device buffer written by any call of
 * this library may be passed to any other call — of the same handle, of another handle, or of no handle (pfd_ew_*) —
 * as soon as the first has returned, and may be freed or overwritten then.  Nothing is left in flight between calls;
 * a caller that writes such a buffer with its own kernels synchronises them before it passes the buffer in. */

/* element dtype codes (payloads and index exports) */
#define PFD_I32 1
#define PFD_U32 2
#define PFD_I64 3
#define PFD_F32 4
#define PFD_F64 5
/* payload-only codes (pfd_fillnodata*): uint64, and the narrow integer dtypes, whose values travel WIDENED in int32
 * lanes (data, out and halo seeds are int32 arrays holding int8 / uint8 / int16 / uint16 values) */
#define PFD_U64 6
#define PFD_I8 7
#define PFD_U8 8
#define PFD_I16 9
#define PFD_U16 10

/* accumulation direction: streams.accuflux (up) / streams.accuflux_ds (down) */
#define PFD_UP 0
#define PFD_DOWN 1
#define PFD_BOTH 2 /* pfd_segment_slope only: fixed_length_slope around the outlet */

/* fillnodata: how the upstream values meet at a confluence (direction "down") */
#define PFD_FILL_MAX 0
#define PFD_FILL_MIN 1
#define PFD_FILL_SUM 2

typedef struct pfd_raster pfd_raster;

/* ---- library / device --------------------------------------------------------------- */
int pfd_abi_version(void);
const char *pfd_last_error(void);
int pfd_device_count(int *count);
/* device memory helpers so that a ctypes caller can keep rasters resident in HBM without
 * any other GPU library (bench.py uses these). */
int pfd_malloc(int device, size_t bytes, void **ptr);
int pfd_free(int device, void *ptr);
/* pfd_malloc / pfd_free on the library's own caching allocator — a reserved arena first (pfd_reserve), then the cache of
 * freed blocks by size class, hipMalloc last: blocks for results that come and go with every call (the per-cell arrays of
 * pyflwdir_amd.DeviceArray), which must not meet hipMalloc / hipFree of multi-GiB blocks in a steady state (0.2 ms or
 * seconds each; profiles/resident_chain_30000.txt).  The block is rounded up to its size class, is at least 256-byte
 * aligned and is valid wherever a pfd_malloc block is; it must be released with pfd_free_pooled, which waits until the
 * device is done with it and hands it to the next taker, the library's working buffers included.  That wait is for the
 * calling thread's last handle stream (or the whole device when it has none), NOT for the null stream the pfd_ew_* calls
 * run on: releasing a block those calls wrote is safe only because each of them synchronises before it returns (the
 * ordering rule above).  A form of the elementwise calls that returned before its kernels finish would have to make this
 * call wait for the null stream as well. */
int pfd_malloc_pooled(int device, size_t bytes, void **ptr);
int pfd_free_pooled(int device, void *ptr);
int pfd_memcpy_h2d(int device, void *dst_dev, const void *src_host, size_t bytes);
int pfd_memcpy_d2h(int device, void *dst_host, const void *src_dev, size_t bytes);
int pfd_device_synchronize(int device);
/* the library caches freed HBM blocks for reuse; pfd_trim returns them to the driver
 * (device < 0: all devices) */
int pfd_trim(int device);
/* Reserve `bytes` of HBM on `device` as ONE arena that the library's working buffers (>= 1 MiB) are carved from before
 * anything else is tried: after this call a steady state never calls hipMalloc, whose latency for multi-GiB blocks is
 * unpredictable on this hardware (0.2 ms or seconds; DESIGN.md "allocation").  May be called more than once (more
 * arenas); requests that do not fit fall back to the class cache / hipMalloc.  bytes == 0 releases the device's arenas
 * that hold no live block.  Callers that time first calls (bench.py, a serving process) reserve before they start. */
int pfd_reserve(int device, size_t bytes);
/* allocator counters since the process started: [0] hipMalloc calls, [1] exact-class cache hits, [2] near-fit cache hits,
 * [3] blocks carved from reserved arenas, [4] idle cached bytes, [5] reserved bytes, [6] of them free, [7] live blocks */
int pfd_alloc_stats(int64_t out[8]);
/* free and total HBM of `device` in bytes (hipMemGetInfo): out[0] free, out[1] total.  The Python front end sizes its
 * default arena with it (pyflwdir_amd/_hip.py ensure_reserved). */
int pfd_mem_info(int device, int64_t out[2]);
/* Host <-> device traffic of the calling thread's API calls since the last call with reset != 0 (§8d "report H2D/D2H
 * separately"): out[0] bytes uploaded from PFD_HOST arguments, out[1] ms spent in those uploads (wall clock of the
 * staging calls), out[2] bytes downloaded into PFD_HOST results, out[3] ms of the downloads (from the moment the stream
 * is idle, i.e. compute excluded), out[4] ms the host spent pre-faulting result pages (runs beside the kernels),
 * out[5] number of host results.  A result buffer of >= 64 MiB is touched by a few host threads while the kernels run
 * (first-touch page faults bound a copy into fresh pages at ~15 GB/s on this host; into touched pages it runs at
 * ~50 GB/s), one byte per page, read and written back unchanged. */
int pfd_transfer_stats(double out[6], int reset);

/* ---- raster handle -------------------------------------------------------------------
 * pfd_raster_create: replaces core_d8.from_array (reference pyflwdir/core_d8.py:42-67) as the
 * constructor of the device-side graph.  `d8` holds nrow*ncol uint8 D8 codes (1 E, 2 SE,
 * 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE, 0/255 pit, 247 nodata; core_d8.py:14-19).  Cells
 * whose target lies outside the raster or on a nodata cell become pits (core_d8.py:57-63).
 * Any other value -> PFD_EBADCODE (the reference only accepts such rasters with
 * check_ftype=False and then decodes them with log2 arithmetic the device path does not
 * imitate).  Fails with PFD_ENOPITS when no pit exists (reference pyflwdir/flwdir.py:126).
 * Rasters of more than 4294967294 cells (32-bit device indices) are accepted for
 * pfd_upstream_area_cell only (LDS-tiled path, e.g. 90000 x 90000 on one 288 GB GPU). */
int pfd_raster_create(const uint8_t *d8, int64_t nrow, int64_t ncol, int memspace, int device,
                      pfd_raster **out);
int pfd_raster_destroy(pfd_raster *h);
/* A flow graph given by its downstream indices (idx_dtype PFD_I32 / PFD_U32 / PFD_I64; -1 cast = nodata,
 * own index = pit) whose links are NOT restricted to the 8 neighbours: NEXTXY rasters (reference
 * pyflwdir/core_nextxy.py:41-68) and upscaled networks (FlwdirRaster(idxs_ds=...), pyflwdir.py:1079-1085).
 * Served by the general level engine (upstream CSR + one launch per level): ordering / idxs_seq / rank /
 * upstream_count / upstream_area / accuflux / Strahler and classic order / basins / HAND / main_upstream /
 * stream_distance (real_length: `step_lengths` = n HOST float32, one per cell); the tile engines, the
 * multi-GPU entry points, ucat_area, floodplains and snap return PFD_EUNSUPPORTED on such a handle. */
int pfd_raster_create_general(const void *idxs_ds, int idx_dtype, int64_t nrow, int64_t ncol, int memspace, int device,
                              pfd_raster **out);
/* One row block of a raster that is tiled over several GPUs (Multi-GPU): `d8` holds
 * halo_top + own_rows + halo_bot rows; the halo rows (0 or 1 each) are copies of the adjacent
 * rows of the neighbouring blocks and are only used to decide where flow leaves the block.
 * Block handles support pfd_upstream_area_cell_blocks / pfd_upstream_area_cell_dist only. */
int pfd_raster_create_block(const uint8_t *d8, int64_t own_rows, int64_t ncol, int halo_top, int halo_bot,
                            int memspace, int device, pfd_raster **out);
/* Same raster / row block (halo_top = halo_bot = 0: a whole raster), but decoding, the pit rule,
 * validation and the counts are DEFERRED to the first operation on the handle: fused into the
 * first tile pass of pfd_upstream_area_cell (and its _blocks/_dist/_begin forms), done by a
 * separate pass for every other entry point.  PFD_EBADCODE / PFD_ENOPITS are then returned by
 * that operation instead of by this call, and pfd_raster_info reports n_valid = n_pits = -1
 * until then.  With PFD_DEVICE the buffer is referenced, not copied: it must stay valid and
 * unmodified until the first operation on the handle has returned.
 * Mirrors from_array(..., check_ftype=False) (reference pyflwdir/pyflwdir.py:93-100) in that the
 * constructor does no validation pass; unlike it, invalid codes are still rejected later. */
int pfd_raster_create_deferred(const uint8_t *d8, int64_t own_rows, int64_t ncol, int halo_top, int halo_bot,
                               int memspace, int device, pfd_raster **out);
/* Normalises and validates a deferred handle now (no-op on any other handle). */
int pfd_raster_validate(pfd_raster *h);

/* info[0]=nrow [1]=ncol [2]=n_valid [3]=n_pits [4]=n_seq (cells draining to a pit; -1 until
 * the cells are ordered) [5]=n_levels (max rank + 1; -1 until ordered) [6]=device
 * [7]=bytes of HBM held by the handle */
int pfd_raster_info(pfd_raster *h, int64_t info[8]);

/* FlwdirRaster.add_pits (reference pyflwdir/flwdir.py:261-279): turn the given cells into
 * pits and invalidate the ordering.  Indices must address valid cells. */
int pfd_add_pits(pfd_raster *h, const int64_t *idxs, int64_t k);

/* ---- index exports (public attributes of FlwdirRaster) ------------------------------- */
/* idxs_ds in the reference's index dtype (PFD_I32/PFD_U32/PFD_I64; pyflwdir.py:105-127):
 * -1 (cast) on nodata, own index on pits.  core_d8.from_array, core_d8.py:42-67. */
int pfd_idxs_ds(pfd_raster *h, int idx_dtype, void *out, int memspace);
/* pit indices ascending; out has n_pits entries.  core_d8.py:62 / core.pit_indices */
int pfd_idxs_pit(pfd_raster *h, int idx_dtype, void *out, int memspace);
/* core.upstream_count (reference pyflwdir/core.py:50-61): int8 in-degree, -9 on nodata;
 * `mask` (uint8, may be NULL) restricts the contributing cells. */
int pfd_upstream_count(pfd_raster *h, const uint8_t *mask, int8_t *out, int memspace);
/* Flwdir.order_cells("walk") (reference pyflwdir/flwdir.py:231-250): build the level
 * structure (cells grouped by rank) that every sweep below uses.  Called implicitly. */
int pfd_order_cells(pfd_raster *h);
/* core.idxs_seq (reference pyflwdir/core.py:87-117): the exact breadth-first order of the
 * reference (pits ascending, then each dequeued cell's upstream cells ascending); out has
 * n_seq entries.  A raster beyond 2^32 - 2 cells (the int64 rung of pyflwdir.py:105-127) takes idx_dtype PFD_I64
 * only: built without the level structure from the tiled rank query and a level-by-level expansion with 64-bit queue
 * entries (csrc/order64.hip); `out` must hold n_valid entries, n_seq of them are written (pfd_raster_info afterwards) —
 * cells that never reach a pit are left out, found by a walk from the pits with one host look per level. */
int pfd_idxs_seq(pfd_raster *h, int idx_dtype, void *out, int memspace);
/* General idxs_ds graphs only: install the cell sequence the sweeps follow.  Flwdir.order_cells("sort")
 * (reference pyflwdir/flwdir.py:231-245; the only ordering of NEXTXY rasters, pyflwdir.py:292-297) sorts the
 * cells by rank with numpy's argsort, and the serial loops add upstream cells in the reverse order of that
 * sequence — a float accumulation depends on it.  `seq`: HOST array of n_seq indices, ordered by rank, every
 * cell that drains to a pit exactly once (anything else: PFD_EINVAL).  seq == NULL with n_seq == 0 forgets an
 * installed sequence: the sweeps (and pfd_idxs_seq) are back on the breadth-first order of core.idxs_seq.
 * pfd_add_pits forgets it as well (it describes the graph before the edit). */
int pfd_set_idxs_seq(pfd_raster *h, int idx_dtype, const void *seq, int64_t n_seq);
/* core.rank (reference pyflwdir/core.py:17-47): int32 distance to the pit, -1 for cells that
 * do not drain to a pit, -9999 on nodata.  Beyond 2^32 - 2 cells: the tiled rank query; a raster with cells that never
 * reach a pit is walked from its pits instead (slower: a host look per level), so that those cells read -1. */
int pfd_rank(pfd_raster *h, int32_t *out, int memspace);

/* ---- sweeps ---------------------------------------------------------------------------- */
/* FlwdirRaster.upstream_area(unit="cell") (reference pyflwdir/pyflwdir.py:770-801): int32
 * upstream cell count incl. the cell itself, -9999 on nodata cells, cells that do not drain
 * to a pit keep 1.  Fused fast path (no weight array is read). */
int pfd_upstream_area_cell(pfd_raster *h, int32_t *out, int memspace);
/* same result through the generic level-by-level engine (kept for cross-checking) */
int pfd_upstream_area_cell_levels(pfd_raster *h, int32_t *out, int memspace);
/* streams.accuflux / streams.accuflux_ds (reference pyflwdir/streams.py:15-41, :44-70).
 * dtype in {PFD_I32, PFD_I64, PFD_F32, PFD_F64}; `nodata_i` is used for the integer types,
 * `nodata_f` for the float types; has_nodata=0 disables the nodata test (the Python
 * comparison can never match, e.g. NaN).  Children are added in the reference's order
 * (descending linear index), so float results are bit-identical to the serial loop.
 * If mask_invalid != 0 nodata cells of the raster are set to `nodata` afterwards
 * (FlwdirRaster.upstream_area, pyflwdir.py:800). */
int pfd_accuflux(pfd_raster *h, int dtype, const void *data, int64_t nodata_i, double nodata_f,
                 int has_nodata, int direction, int mask_invalid, void *out, int memspace);
/* The same accumulation for a payload that is constant along raster rows: `row_values` is a HOST
 * pointer to nrow values of `dtype` (cell areas of a regular grid depend on the row only —
 * FlwdirRaster.upstream_area(unit != "cell"), reference pyflwdir/pyflwdir.py:770-801 with
 * gis_utils.area_grid, gis_utils.py:388-402 — so no n-element input has to exist or travel). */
int pfd_accuflux_rows(pfd_raster *h, int dtype, const void *row_values, int64_t nodata_i, double nodata_f,
                      int has_nodata, int direction, int mask_invalid, void *out, int memspace);
/* FlwdirRaster.fillnodata (reference pyflwdir/flwdir.py:360-392): a copy of `data` whose nodata cells are filled along
 * the flow directions, over the handle's cell order (core.idxs_seq).
 *   direction PFD_UP:   core.fillnodata_upstream (core.py:120-146) — a nodata cell takes the value of the first valid
 *                       cell on its downstream path; `how` is ignored.
 *   direction PFD_DOWN: core.fillnodata_downstream (core.py:149-188) — a nodata cell takes the first valid value of its
 *                       upstream cells (descending linear index, the serial loop's order) and merges the others with
 *                       `how` (PFD_FILL_MAX / PFD_FILL_MIN / PFD_FILL_SUM; sums wrap in the payload dtype).
 * Valid cells, pits ("up"), nodata cells of the raster and cells that do not drain to a pit keep their value.
 * dtype in {PFD_I32, PFD_U32, PFD_I64, PFD_U64, PFD_F32, PFD_F64} or a narrow code (PFD_I8 ... PFD_U16: int32 lanes);
 * nodata_i (integers; the bits of the value for PFD_U64) / nodata_f (floats) / has_nodata as for pfd_accuflux:
 * has_nodata = 0 returns a copy of `data`.  PFD_EINVAL for a bad direction or how, PFD_EUNSUPPORTED for a dtype code
 * outside the list.  Also on general idxs_ds handles (pfd_raster_create_general), over their (installed) order. */
int pfd_fillnodata(pfd_raster *h, int dtype, const void *data, int64_t nodata_i, double nodata_f, int has_nodata,
                   int direction, int how, void *out, int memspace);
/* OPT-IN, tolerance mode of FlwdirRaster.upstream_area(unit != "cell") on lat/lon grids (reference
 * pyflwdir/pyflwdir.py:770-801: a float64 accumulation of cell areas): `row_values` is a HOST pointer to nrow float64
 * areas, `out` receives n float64 sums, -9999 on nodata cells.  The areas are quantised to 64-bit fixed point (the
 * largest power-of-two scale that keeps the raster's rounded float64 total below 2^63, one bit of headroom; *quantum, if given, receives one unit of it) and
 * accumulated as integers on the LDS-tiled engine of pfd_upstream_area_cell (a cell gets the integer part of its row's
 * scaled area plus its Bresenham share of the fraction, so that any run of consecutive cells of a row is off by less than
 * one quantum): the result does not depend on any execution order, every value is the exact sum of the quantised areas,
 * |error| < upstream cells x quantum in the worst case (relative: <= n_cells / 2^62 x mean / min area, 2.6e-10 at
 * 30000^2, reached at cells with a handful of upstream cells) plus one float64 rounding — NOT bit-identical to the reference's
 * serial float64 sum (pfd_accuflux_rows is).  *used = 0: not taken (cycles, row block, general graph, a value that is not
 * finite and positive or lies below the quantum, a total below 2^-960 whose scale is no finite float64, a supertile the 64-bit LDS form cannot hold); `out` is then undefined, call pfd_accuflux_rows. */
int pfd_upstream_area_rows_fixed(pfd_raster *h, const double *row_values, double *out, int memspace, int *used,
                                 double *quantum);
/* streams.strahler_order (reference pyflwdir/streams.py:228-269); mask uint8 or NULL. */
int pfd_strahler(pfd_raster *h, const uint8_t *mask, uint8_t *out, int memspace);
/* basins.basins + core.fillnodata_upstream (reference pyflwdir/basins.py:12-18,
 * pyflwdir/core.py:120-146): `outlets` are k linear indices (host memory, always), `ids`
 * their k labels of `id_size` bytes each (1, 2, 4 or 8; no zeros).  out: n labels. */
int pfd_basins(pfd_raster *h, const int64_t *outlets, const void *ids, int64_t k, int id_size,
               void *out, int memspace);
/* dem.height_above_nearest_drain (reference pyflwdir/dem.py:299-330): drain uint8 (==1 is
 * drain), elevtn PFD_F32 or PFD_F64, out float64 (-9999 off the sequence). */
int pfd_hand(pfd_raster *h, const uint8_t *drain, int elev_dtype, const void *elevtn, double *out,
             int memspace);

/* ---- SURVEY 8(f)-1 -------------------------------------------------------------------------
 * core.main_upstream (reference pyflwdir/core.py:191-219; Flwdir.main_upstream flwdir.py:252-258):
 * per cell the linear index of the upstream cell with the largest `uparea` (payload dtype
 * PFD_I32 / PFD_I64 / PFD_F32 / PFD_F64; strictly larger than upa_min, cast to that dtype, and
 * than every upstream cell of lower index), the index dtype's missing value (-1 / 0xFFFFFFFF)
 * for headwaters and nodata cells.  out: n indices of idx_dtype. */
int pfd_main_upstream(pfd_raster *h, int dtype, const void *uparea, double upa_min, int idx_dtype, void *out,
                      int memspace);
/* arithmetics.upstream_sum (reference pyflwdir/arithmetics.py:147-169; Flwdir.upstream_sum flwdir.py:412-433):
 * per cell the sum of `data` over the cells directly upstream, in the payload dtype (int wrap-around, float
 * addition in ascending cell index like the reference's loop); cells whose own or downstream value is `nodata`
 * get nodata in the place the serial loop would write it; 0 elsewhere (headwaters, nodata cells).  has_nodata = 0:
 * no value compares equal to the missing value (NaN, or not representable in the payload dtype). */
int pfd_upstream_sum(pfd_raster *h, int dtype, const void *data, int64_t nodata_i, double nodata_f, int has_nodata,
                     void *out, int memspace);
/* streams.stream_order, the classic "bottom up" order (reference pyflwdir/streams.py:191-225;
 * Flwdir.stream_order(type="classic") flwdir.py:540-543): uint8; pits 1, tributaries (cells that
 * are not the main upstream cell of a downstream cell with more than one upstream cell inside
 * `mask`) one more than the cell they drain into, 0 outside `mask` (nullable: all cells). */
int pfd_stream_order_classic(pfd_raster *h, int idx_dtype, const void *idxs_us_main, const uint8_t *mask,
                             uint8_t *out, int memspace);
/* streams.stream_distance (reference pyflwdir/streams.py:272-315; FlwdirRaster.stream_distance
 * pyflwdir.py:837-863): distance to the outlet or to the next downstream cell with mask != 0
 * (nullable), -9999 for cells that do not drain to a pit.  real_length == 0: int32 cell counts.
 * real_length != 0: float32; `step_lengths` (HOST pointer, 3 * (2*nrow - 1) floats) holds the
 * length of one step by row sum r0 + r1 and kind {vertical, horizontal, diagonal} — the host
 * evaluates gis_utils.distance (gis_utils.py:452-486), the device only adds in float32. */
int pfd_stream_distance(pfd_raster *h, const uint8_t *mask, int real_length, const float *step_lengths, void *out,
                        int memspace);

/* ---- multi-GPU: upstream_area(unit="cell") on a raster row-tiled over several GPUs -----------
 * In-process form: `hs` are the nblocks row-block handles (top to bottom) of ONE process,
 * outs[b] receives own_rows(b)*ncol int32. */
int pfd_upstream_area_cell_blocks(pfd_raster **hs, int nblocks, int32_t **outs, int memspace);
/* One-process-per-GPU form over RCCL.  Rank 0 obtains a unique id (128 bytes) and ships it to
 * the other ranks by any host-side means; every rank then creates its communicator and calls
 * pfd_upstream_area_cell_dist collectively with its own block (rank r holds block r). */
typedef struct pfd_comm pfd_comm;
int pfd_comm_unique_id(void *id_out, size_t len);
int pfd_comm_create(const void *id, size_t len, int rank, int world, int device, pfd_comm **out);
int pfd_comm_destroy(pfd_comm *c);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) */
int pfd_comm_info(pfd_comm *c, int *nranks, int *rank, int *device);
int pfd_upstream_area_cell_dist(pfd_raster *h, pfd_comm *comm, int32_t *out, int memspace);

/* The exchange step of the iterated row-block collectives (sharded HAND, float accuflux, area-unit upstream_area,
 * Strahler, stream_distance: pyflwdir_amd/dist.py DistributedRaster), device to device over RCCL — SURVEY 8e's
 * "ncclSend/ncclRecv pairs in one ncclGroup": rank k sends the first OWN row of `result_dev` to rank k-1 and the
 * last OWN row to rank k+1 and receives their boundary rows as its new halo values.
 *   result_dev  the block's result on the device (own + halo rows, elem_bytes per cell: 1, 4, 8 or 16)
 *   seed_dev    DEVICE, 2 * ncol elements: the halo values of the next sweep (top halo row, bottom halo row), updated
 *               in place; sides without a neighbour keep their content
 *   counters    in: two local counts; out: [0], [1] their sums over the ranks (one ncclAllReduce), [2] 1 if a
 *               received row differs (bitwise) from the halo values it replaces, [3] the sum of [2] over the ranks
 * No row travels through the host: one stream synchronisation and a 32-byte read-back per exchange.  Every rank
 * must call it (collective).  A rank on which something fails locally (a handle whose halo rows do not fit its rank, a
 * HIP call) still takes part in the send / recv group and in the all-reduce — nobody is left waiting — adds 1 to
 * counters[1] (callers use [1] as "ranks that failed") and returns its own error afterwards.  The block sweeps read `halo_seed_host` from the DEVICE after pfd_set_block_io(h,
 * PFD_DEVICE). */
int pfd_comm_exchange_rows(pfd_comm *comm, pfd_raster *h, const void *result_dev, int elem_bytes, void *seed_dev,
                           int64_t counters[4]);
/* all-gather of `nbytes` host bytes per rank through the device and RCCL (the one-shot boundary records of the sharded
 * basins): out_host receives world * nbytes bytes in rank order.  Collective. */
int pfd_comm_allgather_host(pfd_comm *comm, pfd_raster *h, const void *in_host, size_t nbytes, void *out_host);
/* where the pfd_*_block entry points read their `halo_seed_host` argument from: PFD_HOST (default) or PFD_DEVICE */
int pfd_set_block_io(pfd_raster *h, int seed_memspace);
/* Split-phase form for callers that move the boundary records themselves (MPI, gloo, shared memory ...):
 * begin() runs the local phase and returns this block's record (4*ncol uint32, host memory); finish()
 * takes the records of all blocks in block order (nblocks*4*ncol uint32, host) and completes the pass.
 * *complete = 0 reports cells that never reach a pit (cycles). */
int pfd_upstream_area_cell_begin(pfd_raster *h, int32_t *out, int memspace, uint32_t *record_host);
int pfd_upstream_area_cell_finish(pfd_raster *h, const uint32_t *all_records_host, int nblocks, int block,
                                  int *complete);

/* HAND (reference pyflwdir/dem.py:299-330) of a ROW BLOCK: like pfd_hand on the block's device raster (own rows +
 * halo rows; drain / elevtn / out cover all of them), except that a valid halo cell — the neighbouring block's
 * boundary cell — takes its height from `halo_seed_host` (HOST, 2 * ncol doubles: top halo row, bottom halo row)
 * instead of being computed.  A path that leaves the block therefore continues the neighbour's sum with the same
 * operands in the same order: bit-identical to the whole raster once the seeds are the neighbour's final values.
 * The caller iterates (pyflwdir_amd/dist.py DistributedRaster.hand): seeds start as -inf ("not known yet", which
 * every sum that depends on it inherits), the blocks exchange their boundary rows, until no owned cell is -inf.
 * update != 0: `out` holds the result of an earlier call (other seeds); only its -inf cells are recomputed (collected
 * and relaxed to a fixpoint; a full sweep again when they are more than 1/16 of the block).
 * boundary_rows_host (nullable): receives the first and the last OWN row (2 * ncol doubles); n_unknown (nullable):
 * the number of own cells that are still -inf. */
int pfd_hand_block(pfd_raster *h, const uint8_t *drain, int elev_dtype, const void *elevtn,
                   const double *halo_seed_host, int update, double *out, int memspace, double *boundary_rows_host,
                   int64_t *n_unknown);

/* Up-sweeps of a ROW BLOCK — accuflux (reference pyflwdir/streams.py:15-41, direction "up") and Strahler order
 * (streams.py:228-269) — for rasters cut into row blocks (several GPUs, or one GPU and more than 2^32 - 2 cells).
 * Like pfd_accuflux / pfd_strahler on the block's device raster (own rows + halo rows; data / mask / out cover all of
 * them), except that a valid halo cell — the neighbouring block's boundary cell — has the value given in
 * `halo_seed_host` (HOST, 2 * ncol elements of the result type: top halo row, bottom halo row).  A halo cell that drains
 * into the block is added by its downstream cell in the serial loop's position (upstream cells in descending linear
 * index), so floats come out bit-identical to the whole raster once the seeds are the neighbours' final rows.  The caller
 * iterates (pyflwdir_amd/dist.py up_blocks): exchange the boundary rows and sweep again until no row changes.
 *   direction:   PFD_UP, or PFD_DOWN (streams.accuflux_ds, streams.py:44-70: values travel upstream; a halo cell the
 *                block drains into then holds the neighbour's value, and the same exchange-until-stable applies).
 *   by_row != 0: `data` holds one value per ROW of the device raster (HOST; upstream_area(unit="km2") on lat/lon grids).
 *   verify != 0: nothing is computed; `out` holds a result, *n_bad receives the number of own cells whose value is not
 *                the one their upstream cells (halo seeds included) give — the all-cell check of a blocked result.
 *   boundary_rows_host (nullable): receives the first and the last OWN row (2 * ncol elements). */
/* Repeated up-sweeps of one block (the exchange-until-stable iteration above) — what the next pfd_accuflux_block
 * (direction PFD_UP) / pfd_strahler_block call on `h` keeps or reuses, with result and payload in DEVICE memory:
 *   0 (default)  nothing is kept (a kept sweep is released);
 *   1            a full sweep whose per-chain arrays and seeds stay on the handle (8-16 bytes per trunk slot);
 *   2            `out` still holds the result of the kept sweep of the same operation, payload and mask: only the
 *                chains below a halo seed that CHANGED are folded again (no tile pass, no pass over the raster: the
 *                cost follows the cells the changed seeds reach).  Falls back to mode 1 when there is no kept sweep
 *                of this operation into this buffer.  Results are the full sweep's, bit for bit.
 * Handles whose block has no exact-order plan (PFD_BLOCK_LEVELS) ignore the mode.  With mode 1 or 2 a call whose
 * memspace is not PFD_DEVICE returns PFD_EINVAL (the kept sweep refers to `out` by address). */
int pfd_set_block_update(pfd_raster *h, int mode);
int pfd_accuflux_block(pfd_raster *h, int dtype, const void *data, int by_row, int64_t nodata_i, double nodata_f,
                       int has_nodata, int direction, const void *halo_seed_host, int verify, void *out, int memspace,
                       void *boundary_rows_host, int64_t *n_bad);
int pfd_strahler_block(pfd_raster *h, const uint8_t *mask, const uint8_t *halo_seed_host, int verify, uint8_t *out,
                       int memspace, uint8_t *boundary_rows_host, int64_t *n_bad);
/* fillnodata (reference pyflwdir/flwdir.py:360-392, core.py:120-188) of a ROW BLOCK, like pfd_accuflux_block:
 * `halo_seed_host` holds the neighbours' results on the halo rows (2 * ncol elements of the payload's lane type).
 * direction PFD_DOWN (an up-sweep): a halo cell that drains into the block is merged by its downstream cell in the serial
 * loop's position; PFD_UP (a down-sweep): a halo cell the block drains into holds the neighbour's filled value.  The
 * caller exchanges boundary rows until none changes (pyflwdir_amd/dist.py fillnodata_blocks); `verify`,
 * `boundary_rows_host` and `n_bad` as for pfd_accuflux_block.  pfd_set_block_update does not apply. */
int pfd_fillnodata_block(pfd_raster *h, int dtype, const void *data, int64_t nodata_i, double nodata_f, int has_nodata,
                         int direction, int how, const void *halo_seed_host, int verify, void *out, int memspace,
                         void *boundary_rows_host, int64_t *n_bad);
/* stream_distance (reference pyflwdir/streams.py:272-315) of a row block, like pfd_accuflux_block in direction "down":
 * the halo cells the block drains into hold the neighbour's distances (`halo_seed_host`: 2 * ncol int32, or float32
 * when real_length != 0); `step_lengths` covers the rows of the block's device raster (3 * (2 * nrow - 1) floats: the
 * slice of the whole raster's table that starts at the block's first device row). */
int pfd_stream_distance_block(pfd_raster *h, const uint8_t *mask, int real_length, const float *step_lengths,
                              const void *halo_seed_host, int verify, void *out, int memspace, void *boundary_rows_host,
                              int64_t *n_bad);
/* dem.floodplains (reference pyflwdir/dem.py:333-379) of a row block, like pfd_stream_distance_block: the halo cells the
 * block drains into hold the neighbouring block's floodplain STATE, 16 bytes per cell {float z, float h, int32 flag, int32
 * pad} (z / h: elevation and height threshold of the stream cell that started the floodplain; flag 1 floodplain, 0 not,
 * -1 nodata); `state` (own + halo rows of the block's device raster) is the result, `halo_seed_host` / boundary rows hold
 * 2 * ncol such records.  `is_stream` / `stream_h` as in pfd_floodplains.  Iterated by pyflwdir_amd/dist.py
 * floodplains_blocks until no boundary row changes: floodplains on rasters beyond 2^32 - 2 cells. */
int pfd_floodplains_block(pfd_raster *h, int elev_dtype, const void *elevtn, const uint8_t *is_stream, const float *stream_h,
                          const void *halo_seed_host, int verify, void *state, int memspace, void *boundary_rows_host,
                          int64_t *n_bad);
/* The int8 result of dem.floodplains (1 floodplain, 0 not, -1 off the sequence; dem.py:333-379) for the block's OWN rows,
 * from the DEVICE-resident `state` of pfd_floodplains_block: own_rows * ncol bytes into `out` (host or device) — a caller
 * that assembles the raster on the host moves 1 byte per cell instead of the 16-byte state records. */
int pfd_floodplains_block_flags(pfd_raster *h, const void *state_dev, int8_t *out, int memspace);
/* Classic stream order (reference pyflwdir/streams.py:191-225 with core.main_upstream, core.py:191-219) over row blocks.
 * pfd_trib_info_block: one byte per cell of the block's device raster — low 4 bits the slot (0-7; 15 none) of the cell's
 * main upstream cell (largest `uparea` > upa_min, first in ascending index), bit 4 set when more than one upstream cell
 * lies inside `mask` (nullable) — from the upstream masks that include the halo cells.  The byte of a HALO cell is
 * incomplete (its upstream cells lie beyond the block): the caller replaces the halo rows of `tinfo` with the
 * neighbouring blocks' boundary rows, then pfd_stream_order_classic_block sweeps down- to upstream with the halo cells
 * the block drains into holding the neighbour's orders (`halo_seed_host`: 2 * ncol uint8), like
 * pfd_stream_distance_block; iterated until no boundary row changes (pyflwdir_amd/dist.py classic_blocks). */
int pfd_trib_info_block(pfd_raster *h, int dtype, const void *uparea, double upa_min, const uint8_t *mask, uint8_t *tinfo,
                        int memspace);
int pfd_stream_order_classic_block(pfd_raster *h, const uint8_t *tinfo, const uint8_t *mask, const uint8_t *halo_seed_host,
                                   int verify, uint8_t *out, int memspace, uint8_t *boundary_rows_host, int64_t *n_bad);

/* basins (reference pyflwdir/basins.py:12-18, core.py:120-146) on a raster row-tiled over several GPUs /
 * processes, split-phase like pfd_upstream_area_cell_begin/_finish (Multi-GPU): `outlets` are k
 * linear indices INTO THE BLOCK'S OWN ROWS (r * ncol + c, r counted from the block's first own row), `ids`
 * their labels (id_size bytes each, no zeros).  begin() runs the local label query and returns the block's
 * boundary record (6 * ncol uint32, host); finish() takes the records of all blocks in block order
 * (nblocks * 6 * ncol uint32, host), resolves the paths that leave the block and writes the own_rows * ncol
 * labels to the `out` given to begin().  *complete = 0 reports a cycle through several blocks. */
int pfd_basins_begin(pfd_raster *h, const int64_t *outlets, const void *ids, int64_t k, int id_size, void *out,
                     int memspace, uint32_t *record_host);
int pfd_basins_finish(pfd_raster *h, const uint32_t *all_records_host, int nblocks, int block, int *complete);

/* ---- the step before the path (DEM -> D8) -------------------------------------------------
 * dem.fill_depressions (reference pyflwdir/dem.py:17-143; from_dem pyflwdir/pyflwdir.py:51-102): priority flood
 * (Wang & Liu 2006) with the reference's heap order (float32 elevation, boundary flag, row, column).  HOST
 * function (inherently sequential), all pointers are host pointers.  dtype PFD_F32 / PFD_F64 / PFD_I32;
 * nodata NaN selects isnan(); max_depth < 0: fill everything; outlets_min != 0: one outlet at the lowest edge
 * cell; has_elv_max: edge outlets only up to elv_max; idxs_pit (nullable): user outlets instead of the edge;
 * connectivity 4 or 8.  elev_out: filled elevation (dtype of the input), d8_out: uint8 D8 codes (247 nodata). */
int pfd_fill_depressions(int dtype, const void *elevtn, int64_t nrow, int64_t ncol, double nodata, double max_depth,
                         int outlets_min, int has_elv_max, double elv_max, const int64_t *idxs_pit, int64_t npit,
                         int connectivity, void *elev_out, uint8_t *d8_out);

/* ---- SURVEY 8(f)-4 --------------------------------------------------------------------------------
 * subgrid.ucat_area (reference pyflwdir/subgrid.py:51-93; FlwdirRaster.ucat_area pyflwdir.py:1159-1191): unit
 * catchment map and area.  `idxs_out`: k outlet cells (HOST; < 0 = missing).  map_out: n labels of map_dtype
 * (PFD_I32/U32/I64; label i+1 for outlet i, 0 elsewhere).  area_dtype PFD_I32: cell counts (area_rows NULL);
 * PFD_F32/PFD_F64: `area_rows` = nrow HOST values, the area of a cell of that row; area_out: k HOST values of
 * area_dtype (-9999 for missing outlets), float sums accumulated in the reference's (idxs_seq) order.
 * Any raster size (round 6): beyond 2^32 - 2 cells the label query runs on the whole raster (tiles and slots, 32-bit
 * values) and the float sums walk the 64-bit sequence (csrc/order64.hip) in sorted pieces, bit-identical to the
 * reference's loop; a raster of that size WITH cycles returns PFD_EUNSUPPORTED (its label query needs the level
 * engine's 32-bit order) — as does pfd_basins, which otherwise runs at any size too. */
int pfd_ucat_area(pfd_raster *h, const int64_t *idxs_out, int64_t k, int map_dtype, void *map_out, int memspace,
                  int area_dtype, const void *area_rows, void *area_out);
/* subgrid.ucat_volume (reference pyflwdir/subgrid.py:96-142; FlwdirRaster.ucat_volume pyflwdir.py:1193-1225): unit
 * catchment map and floodplain volume per depth.  `idxs_out`, `map_dtype`, `map_out` and `area_rows` as for pfd_ucat_area
 * (area_dtype PFD_F32 / PFD_F64); `hand`: n values of hand_dtype (PFD_F32 / PFD_F64); `depths`: ndepths HOST values of
 * depth_dtype (PFD_F32 / PFD_F64); vol_out: ndepths x k values of depth_dtype, depth-major (-9999 for missing outlets).
 * `memspace` covers hand, map_out and vol_out.  The arithmetic is the reference's, type by type: dh = max(0, depth - hand)
 * in the common type of depths and hand, area * dh in the common type of all three, the running column rounded to
 * depth_dtype after every add, cells added in idxs_seq order.  32-bit cell indices, D8 handles. */
int pfd_ucat_volume(pfd_raster *h, const int64_t *idxs_out, int64_t k, int map_dtype, void *map_out, int hand_dtype,
                    const void *hand, int area_dtype, const void *area_rows, int depth_dtype, const void *depths,
                    int64_t ndepths, void *vol_out, int memspace);
/* ---- river segments between unit-catchment outlets (csrc/subgrid.hip) ---------------------------------------------
 * Common arguments: `idxs_out` k outlet cells (HOST int64; < 0 = missing: the result holds nodata there; repeats allowed);
 * `direction` PFD_DOWN follows the handle's downstream links, PFD_UP the caller's `idxs_us_main` (n indices of idx_dtype,
 * the dtype's -1 = none; may be NULL for PFD_DOWN); `mask` uint8 (nullable): a walk stops before a cell where it is 0.
 * `memspace` covers idxs_us_main, mask, the per-cell payloads and `out` (k values).  An index outside the raster and a
 * walk that does not end within n steps (a cycle) return PFD_EINVAL.  D8 handles with 32-bit cell indices.
 * pfd_segment_length — subgrid.segment_length (subgrid.py:145-205; FlwdirRaster.subgrid_rivlen pyflwdir.py:1227-1274):
 *   the walk steps ONTO the next outlet; out = |distnc[last] - distnc[outlet]| in dist_dtype (PFD_I32 cells with nodata
 *   -9999, PFD_F32 metres with nodata -9999.0).
 * pfd_segment_slope — subgrid.segment_slope and fixed_length_slope with lstsq=False (subgrid.py:414-559;
 *   FlwdirRaster.subgrid_rivslp pyflwdir.py:1276-1342): PFD_UP / PFD_DOWN: |dz / dx| between the outlet and the last cell
 *   BEFORE the next outlet, in elev_dtype (PFD_F32 / PFD_F64), 0 for a one-cell segment; PFD_BOTH: down while
 *   distnc > distnc[outlet] - length / 2 (or a pit), then up the main stem while distnc < distnc[outlet] + length / 2,
 *   float32.  `distnc`: n float32.  No mask: the interpreted reference never honours it (`mask[i] is False`).  The
 *   least-squares form is not offered: its float32 powf and its cancelling denominator cannot be reproduced.
 * pfd_segment_average — subgrid.segment_average with arithmetics._average (subgrid.py:208-272, arithmetics.py:17-29;
 *   FlwdirRaster.subgrid_rivavg pyflwdir.py:1344-1398): the weighted mean of the cells from the outlet to the last cell
 *   BEFORE the next outlet, skipping `nodata` (NaN: isnan); data PFD_F32 / PFD_F64, `weights` of weight_dtype (NULL: ones of
 *   that dtype); sums in the reference's accumulator types; nodata where the weights sum to 0.
 * pfd_segment_median — subgrid.segment_median (subgrid.py:277-337): the median of the same cells without nodata and NaN,
 *   the mean of the two middle values in the data's dtype for an even count, NaN for a segment without values. */
int pfd_segment_length(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                       const void *idxs_us_main, const uint8_t *mask, int dist_dtype, const void *distnc, void *out,
                       int memspace);
int pfd_segment_slope(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                      const void *idxs_us_main, int elev_dtype, const void *elevtn, const float *distnc, double length,
                      void *out, int memspace);
int pfd_segment_average(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                        const void *idxs_us_main, const uint8_t *mask, int dtype, const void *data, int weight_dtype,
                        const void *weights, double nodata, void *out, int memspace);
int pfd_segment_median(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                       const void *idxs_us_main, const uint8_t *mask, int dtype, const void *data, double nodata, void *out,
                       int memspace);
/* ---- outlets derived from the network: mark -> list in sequence order -> (number, fill) -----------------------------
 * Three calls of the reference are one primitive (csrc/outlets.hip): mark cells by a rule that looks at the cell and its
 * downstream cell, list the marked cells in the order of core.idxs_seq (only cells IN the sequence count: a cell on or
 * above a cycle is never an outlet, as in the reference, whose loops run over `seq`), and for the sub-basins number the
 * list 1..k and fill the numbers upstream with the label query of pfd_basins.  The sequence stays on the device.
 * Common arguments: `idx_dtype` (PFD_I32 / PFD_U32 / PFD_I64) is the type of `idxs_out`, which has room for `cap`
 * entries; *k_out receives the number of outlets.  k > cap is NOT an error: PFD_OK, the list (and `lbs_out`) are left
 * unwritten, everything else is complete — the caller repeats the call with cap >= k.  `memspace` covers the per-cell
 * input, the per-cell output and the lists alike.  On D8 handles of any size (beyond 2^32 - 2 cells over the 64-bit
 * sequence of csrc/order64.hip; PFD_EUNSUPPORTED there for a raster with cycles, like pfd_basins) and on general
 * idxs_ds handles (over their installed order, if any); not on row-block handles.
 *
 * pfd_subbasins_streamorder — basins.subbasins_streamorder (reference pyflwdir/basins.py:67-103; FlwdirRaster.
 *   subbasins_streamorder pyflwdir.py:601-629): `strord` holds n values of `dtype` (PFD_U8, PFD_I32, PFD_U32 or PFD_I64);
 *   a cell is an outlet iff strord >= min_sto and (it is a pit or its downstream cell has another strord); outlets are
 *   listed in REVERSED sequence order; map_out: n int32, the list position + 1 of the first outlet on the cell's
 *   downstream path (itself included), 0 if there is none.  min_sto is taken as given (the reference's negative form,
 *   max(strord) + min_sto, is the caller's to resolve).
 * pfd_outflow_idxs — core.outflow_idxs (core.py:501-514; FlwdirRaster.outflow_idxs pyflwdir.py:820-835): `region` uint8
 *   (!= 0 inside); the cells of the region that are a pit or drain to a cell outside it, and have no other such cell
 *   further down their flow path (one label fill of the candidates); FORWARD sequence order.
 * pfd_basin_outlets — regions.region_outlets (regions.py:129-163; FlwdirRaster.basin_outlets pyflwdir.py:720-740):
 *   `regions` holds n labels of `dtype` (PFD_I32, PFD_U32, PFD_I64 or PFD_U64); a cell is an outlet iff its label is > 0
 *   and (it is a pit or its downstream cell has another label).  lbs_out (cap labels of `dtype`) and idxs_out are
 *   sorted by label; outlets of one label keep their reversed sequence order (the reference sorts with an unstable
 *   argsort: their order is unspecified there). */
int pfd_subbasins_streamorder(pfd_raster *h, int dtype, const void *strord, int64_t min_sto, int idx_dtype, void *idxs_out,
                              int64_t cap, int64_t *k_out, int32_t *map_out, int memspace);
int pfd_outflow_idxs(pfd_raster *h, const uint8_t *region, int idx_dtype, void *idxs_out, int64_t cap, int64_t *k_out,
                     int memspace);
int pfd_basin_outlets(pfd_raster *h, int dtype, const void *regions, int idx_dtype, void *idxs_out, void *lbs_out,
                      int64_t cap, int64_t *k_out, int memspace);
/* ---- the rest of the BASINS section (csrc/basins_ext.hip) -----------------------------------------------------------
 * Lists follow the conventions of pfd_outflow_idxs (cap, *k_out always written, the list only when it fits).
 * pfd_interbasin_mask — basins.interbasin_mask (basins.py:25-64; FlwdirRaster.interbasin_mask pyflwdir.py:742-766):
 *   `region` uint8 (!= 0 inside), `stream` uint8 or NULL; out: n uint8 (0 / 1).  A cell of the sequence is set iff it
 *   lies in the region, the basin of its pit holds a stream cell (no `stream`: always) and no cell on its path down to
 *   the pit lies outside the region while draining into it; a cell off the sequence keeps stream && region.
 * pfd_inflow_idxs — core.inflow_idxs (core.py:485-497; FlwdirRaster.inflow_idxs pyflwdir.py:804-818): the cells outside
 *   `region` that drain into it and whose flag — handed down from the child that comes first in the sequence — is
 *   still set; REVERSED sequence order.
 * pfd_basin_bounds — regions.region_slices (regions.py:57-82) of a label map of `dtype` (PFD_I32, PFD_U32, PFD_I64 or
 *   PFD_U64): lbs_out = the k sorted unique labels > 0 (cap labels of `dtype`), bounds_out = 4 * k int64 as
 *   [row_min[k], row_max[k], col_min[k], col_max[k]] (inclusive).  Needs no flow directions: any handle of the shape.
 * pfd_subbasins_pfafstetter — basins.subbasins_pfafstetter (basins.py:106-191; FlwdirRaster.subbasins_pfafstetter
 *   pyflwdir.py:631-663): `uparea` n values of `dtype` (PFD_I32 / PFD_I64 / PFD_F32 / PFD_F64) or NULL = the upstream
 *   cell count; the stream mask is uparea >= upa_min; `idxs_us_main` n int64 (-1 = none) or NULL = the main upstream
 *   cells by upstream cell count; `idxs_pit`: npits cells, always a HOST list; depth 1 .. 8.  map_out: n int32 codes;
 *   idxs_out: the outlets in the reference's append order.  Both of the reference's np.argsort calls are STABLE sorts
 *   on the negated key here (ties keep list order; the reference leaves them unspecified).  32-bit cell indices only:
 *   beyond 2^32 - 2 cells PFD_EUNSUPPORTED (pfd_main_upstream / pfd_stream_order_classic have no one-handle form). */
int pfd_interbasin_mask(pfd_raster *h, const uint8_t *region, const uint8_t *stream, uint8_t *out, int memspace);
int pfd_inflow_idxs(pfd_raster *h, const uint8_t *region, int idx_dtype, void *idxs_out, int64_t cap, int64_t *k_out,
                    int memspace);
int pfd_basin_bounds(pfd_raster *h, int dtype, const void *labels, void *lbs_out, int64_t *bounds_out, int64_t cap,
                     int64_t *k_out, int memspace);
int pfd_subbasins_pfafstetter(pfd_raster *h, int dtype, const void *uparea, double upa_min, int depth,
                              const int64_t *idxs_us_main, const int64_t *idxs_pit, int64_t npits, int idx_dtype,
                              void *idxs_out, int64_t cap, int64_t *k_out, int32_t *map_out, int memspace);
/* ---- sub-basins of a minimum area (csrc/subbasins_area.hip) ----------------------------------------------------------
 * pfd_subbasins_area — basins.subbasins_area (basins.py:194-233; FlwdirRaster.subbasins_area pyflwdir.py:665-692).  Moving
 *   upstream from the pits, a tributary whose area exceeds area_min where what is left of the main stem's area also does
 *   becomes an outlet, and so does a main-stem cell once the area between it and the cell below exceeds area_min.
 *   `uparea`: n values of `dtype` (PFD_I32 / PFD_I64 / PFD_F32 / PFD_F64) or NULL = the upstream cell count (int32).  Every
 *   difference of areas is formed and rounded in that dtype; `compare` says where `> area_min` is evaluated:
 *   PFD_COMPARE_OWN in the areas' dtype, area_min rounded to it once (integer areas: area_min must be one of its values,
 *   PFD_EINVAL otherwise), PFD_COMPARE_F64 in float64.  A NaN area is above nothing.  `idxs_us_main`: n int64 (-1 = none)
 *   or NULL = the main upstream cells by upstream cell count; every entry must be another cell that drains into its cell,
 *   and a cell at which a tributary becomes an outlet must have one (PFD_EINVAL otherwise).
 *   idxs_out: the outlets in sequence order, the pits first — list conventions of pfd_outflow_idxs (`cap`; *k_out is always
 *   written, the list only when it fits).  map_out: n uint32, the list position + 1 of the first outlet on the cell's
 *   downstream path, itself included; 0 off the sequence (nodata, and cells on or above a loop: a raster with loops is
 *   served).  stats_out (nullable): [0] mode 0 = pruned (the cells above area_min are closed downstream: a cell that is
 *   not above it is never followed) / 1 = full, [1] rounds, [2] jobs, [3] lane steps (groups run).  flags:
 *   PFD_SUBAREA_FULL forces the full mode (same result; for tests).  `memspace` covers uparea, idxs_us_main, map_out and
 *   the list.  PFD_EUNSUPPORTED beyond 2^32 - 2 cells, on row-block handles and on general idxs_ds handles: the only
 *   sequence of a general graph is the reference's np.argsort by rank, an unstable sort, so the order of the upstream
 *   cells of one cell — on which this result depends — is unspecified there. */
#define PFD_COMPARE_OWN 0
#define PFD_COMPARE_F64 1
#define PFD_SUBAREA_FULL 1
int pfd_subbasins_area(pfd_raster *h, int dtype, const void *uparea /* nullable */, double area_min, int compare,
                       const int64_t *idxs_us_main /* nullable */, int idx_dtype, void *idxs_out, int64_t cap,
                       int64_t *k_out, uint32_t *map_out, int64_t *stats_out /* nullable, 4 */, int flags, int memspace);
/* ---- stream segments: from outlet lists to segment lists (csrc/streams.hip) ----------------------------------------
 * pfd_streams — streams.streams (reference pyflwdir/streams.py:132-188; FlwdirRaster.streams pyflwdir.py:894-974) as a
 *   CSR triple.  `mask` uint8 (!= 0: stream cell; NULL: every cell).  With nup = the upstream count inside the mask, a
 *   segment starts at every cell of the sequence that lies in the mask and is not walked through by another segment
 *   (nup != 1, or no upstream neighbour that a walk leaves), in REVERSED sequence order; it follows the downstream
 *   links — through cells outside the mask as well — up to and including the first cell with nup > 1, or ends at a pit.
 *   n_out[0] = K segments, n_out[1] = M indices; offsets_out: K + 1 int64 (segment j is idxs_out[offsets[j] ..
 *   offsets[j + 1])), idxs_out: M cells of `idx_dtype` (PFD_I32 / PFD_U32 / PFD_I64), pit_out: K uint8, 1 where the
 *   segment ended at a pit.  The lists are the UNSPLIT segments: the reference's `max_len` pieces and the `[p, p]` entry
 *   it appends after a segment that ends at pit p are slices of this triple and left to the caller.
 *   Conventions of pfd_outflow_idxs: n_out is always written; the three lists are written only when K <= cap_segs and
 *   M <= cap_idxs (not an error otherwise: the caller repeats the call with room; a sizing call passes caps of 0 and
 *   NULL lists); `memspace` covers the mask and all outputs.  On D8 handles and general idxs_ds handles (over their
 *   installed order, if any); not on row-block handles; a raster beyond 2^32 - 2 cells (64-bit cell indices) returns
 *   PFD_EUNSUPPORTED: a list of that many segments is beyond what a caller can hold. */
int pfd_streams(pfd_raster *h, const uint8_t *mask /* nullable */, int idx_dtype, void *idxs_out, int64_t cap_idxs,
                int64_t *offsets_out /* cap_segs + 1 */, uint8_t *pit_out, int64_t cap_segs,
                int64_t n_out[2] /* K segments, M indices */, int memspace);
/* ---- upscaling: a coarse network from a fine D8 raster (csrc/upscale.hip) ------------------------------------------------
 * The data-parallel methods of the reference's upscale.py, on the eager D8 handle's decoded downstream links (a general
 * idxs_ds handle, a row block and a raster beyond 2^32 - 2 cells return PFD_EUNSUPPORTED).  The coarse grid has
 * ceil(nrow / cellsize) x ceil(ncol / cellsize) = n1 cells (the last row and column may be partial); cellsize >= 1.
 * `method`: PFD_UPSCALE_DMM   upscale.dmm  = dmm_exitcell + dmm_nextidx                (upscale.py:66-111, :114-169)
 *           PFD_UPSCALE_EAM   upscale.eam  = eam_repcell + eam_nextidx                 (upscale.py:243-287, :290-335)
 *           PFD_UPSCALE_EAM_PLUS  upscale.eam_plus = ihu(niter=0) = eam_repcell + ihu_outlets + ihu_nextidx
 *                                                                    (upscale.py:1308-1309, :381-434, :437-496)
 * `uparea`: n values of uparea_dtype (PFD_I32 / PFD_F32 / PFD_F64), compared in that type.  The representative / exit cell
 * of a coarse cell is the valid fine cell, a pit or inside the method's selector (the coarse cell's edge, cell_edge
 * upscale.py:41-46; the effective area, effective_area :214-223), with the largest uparea > 0 — the SMALLEST fine index
 * among equals (the reference's ascending scan with a strict >); a NaN never wins; none: the missing value.
 * `effarea_host`: HOST, min(cellsize, nrow) x min(cellsize, ncol) bytes, != 0 where (ri, ci) = (row % cellsize,
 * col % cellsize) lies in the effective area — evaluated by the caller in float64, the device takes no square root;
 * may be NULL for PFD_UPSCALE_DMM.
 * Outputs, n1 entries of idx_dtype (PFD_I32 / PFD_U32 / PFD_I64; -1 cast = missing): idxs_out_out the fine index of each
 * coarse cell's exit (DMM) / representative (EAM) / outlet (EAM+) cell, idxs_ds_out the coarse downstream index.
 * `memspace` covers uparea and both outputs.  Every walk along the fine links is capped at n steps: a fine raster with a
 * cycle returns PFD_EINVAL where the reference's `while True` never returns; so does an EAM+ cell for which the reference
 * would index with its missing value (no outlet within the 8 neighbours and no effective area on the way).
 * pfd_upscale_outlets — subgrid.outlets (reference pyflwdir/subgrid.py:13-48; FlwdirRaster.ucat_outlets pyflwdir.py:
 *   1125-1157): idxs_out_out alone (PFD_UPSCALE_DMM: dmm_exitcell; PFD_UPSCALE_EAM_PLUS: eam_repcell + ihu_outlets;
 *   PFD_UPSCALE_EAM: the representative cells).
 * pfd_upscale_error — upscale.upscale_error (upscale.py:1312-1363; FlwdirRaster.upscale_error pyflwdir.py:1093-1121) on
 *   the FINE handle: `idxs_out` (fine outlet cells) and `idxs_ds_coarse` (coarse downstream indices), k entries of
 *   idx_dtype each; out: k uint8 — 1 where the first outlet cell (or pit) downstream of a cell's outlet is the outlet
 *   of its downstream coarse cell, 0 where not, 255 where either entry is missing.  An entry outside its raster: PFD_EINVAL. */
#define PFD_UPSCALE_DMM 0
#define PFD_UPSCALE_EAM 1
#define PFD_UPSCALE_EAM_PLUS 2
int pfd_upscale(pfd_raster *h, int method, int64_t cellsize, int uparea_dtype, const void *uparea,
                const uint8_t *effarea_host, int idx_dtype, void *idxs_ds_out, void *idxs_out_out, int memspace);
int pfd_upscale_outlets(pfd_raster *h, int method, int64_t cellsize, int uparea_dtype, const void *uparea,
                        const uint8_t *effarea_host, int idx_dtype, void *idxs_out_out, int memspace);
int pfd_upscale_error(pfd_raster *h, int idx_dtype, const void *idxs_out, const void *idxs_ds_coarse, int64_t k,
                      uint8_t *out, int memspace);
/* ---- windows along the flow path (csrc/window.hip) ---------------------------------------------------------------------
 * The calls that look along the flow path around a cell.  D8 handles with 32-bit cell indices (a general idxs_ds handle, a
 * row block and a raster beyond 2^32 - 2 cells return PFD_EUNSUPPORTED).  `memspace` covers every per-cell argument and
 * the result.
 * pfd_downstream — Flwdir.downstream (reference pyflwdir/flwdir.py:394-410): out[x] = data[idxs_ds[x]] for a valid cell (a
 *   pit takes its own value), data[x] for a nodata cell.  A gather of elements of `elem_bytes` = 1, 2, 4 or 8 bytes: any
 *   dtype of those sizes.
 * pfd_moving_average — arithmetics.moving_average (arithmetics.py:67-103) over core._window (core.py:369-397): the window
 *   of a cell is at most n cells down the downstream links (ending at a pit, and BEFORE a cell whose stream order is
 *   greater than the CENTRE cell's when `strord` is given) and at most n cells up `idxs_us_main` (n indices of idx_dtype,
 *   the dtype's -1 = none; every entry must drain into its cell, as pfd_main_upstream's do: PFD_EINVAL otherwise).  `strord`
 *   (nullable): n values of strord_dtype (PFD_U8, PFD_I32, PFD_U32 or PFD_I64), compared as integers.  out = `nodata`
 *   where data == nodata (compared in the data's dtype: a NaN nodata skips no cell); else arithmetics._average over the
 *   window from its farthest upstream to its farthest downstream cell, skipping values == nodata (NaN nodata: isnan):
 *   v += w0 * v0 in the common type of weights and data (the product rounded before the add), w += w0 in the type of the
 *   weights, v / w rounded to the data's dtype, nodata where w == 0.  data PFD_F32 / PFD_F64; `weights` of weight_dtype
 *   (PFD_F32 / PFD_F64), or NULL = float64 ones, as in the reference.  n >= 0; the walks are bounded by n, so a raster with
 *   cycles is served like any other.
 * pfd_moving_median — arithmetics.moving_median (arithmetics.py:106-143): the same window and cell test; np.nanmedian of
 *   the window's values that are neither nodata nor NaN: the middle value, or (a + b) / 2 in the data's dtype for an even
 *   count, NaN for none.  Values are ordered by the total order (-0.0 before 0.0; the reference's np.partition leaves the
 *   order of zeros of both signs unspecified).  Windows of 2n + 1 <= WMAX cells (pfd_debug_window_wmax: 31 for float32, 15
 *   for float64) are sorted in LDS, larger ones in a global workspace of a fixed byte budget that serves the raster in
 *   chunks of cells: no n is refused for its size.
 * pfd_path — core.path / core._trace (core.py:308-437; FlwdirRaster.path pyflwdir.py:443-500): per start cell (`idxs`, k
 *   HOST int64) the cells of the walk along the downstream links (PFD_DOWN) or `idxs_us_main` (PFD_UP; n indices of
 *   idx_dtype), the start cell included, up to and including the first cell where `mask` (uint8, nullable) is set, a pit,
 *   a headwater or a missing link; with has_max_length the walk ends before the step that would make the distance exceed
 *   max_length.  `step_lengths` as for pfd_snap (HOST table, NULL counts cells).  A CSR pair with the conventions of
 *   pfd_streams: *n_out = M cells in all, always written; idxs_out (M cells of idx_dtype), offsets_out (k + 1 int64) and
 *   dist_out (k float64, accumulated in float64 and NOT rounded to float32 as pfd_snap's are) are written only when
 *   M <= cap_idxs (a sizing call passes cap_idxs = 0 and NULL lists).  A start index outside the raster and a walk that
 *   does not end within n_cells steps (a cycle) return PFD_EINVAL.
 * pfd_debug_window_wmax — *wmax = the largest window (2n + 1) the median sorts in LDS for `dtype` (PFD_F32 / PFD_F64). */
int pfd_downstream(pfd_raster *h, int elem_bytes, const void *data, void *out, int memspace);
int pfd_moving_average(pfd_raster *h, int64_t n, int idx_dtype, const void *idxs_us_main, int strord_dtype,
                       const void *strord /* nullable */, int dtype, const void *data, int weight_dtype,
                       const void *weights /* nullable */, double nodata, void *out, int memspace);
int pfd_moving_median(pfd_raster *h, int64_t n, int idx_dtype, const void *idxs_us_main, int strord_dtype,
                      const void *strord /* nullable */, int dtype, const void *data, double nodata, void *out, int memspace);
int pfd_path(pfd_raster *h, const int64_t *idxs, int64_t k, int direction, int idx_dtype,
             const void *idxs_us_main /* nullable for PFD_DOWN */, const uint8_t *mask /* nullable */,
             const double *step_lengths /* nullable */, int has_max_length, double max_length, void *idxs_out,
             int64_t cap_idxs, int64_t *offsets_out /* k + 1 */, double *dist_out /* k */, int64_t *n_out, int memspace);
int pfd_debug_window_wmax(int dtype, int *wmax);
/* dem.floodplains (reference pyflwdir/dem.py:333-379; FlwdirRaster.floodplains pyflwdir.py:1513-1545):
 * `is_stream` uint8 (1 where uparea >= upa_min), `stream_h` float32 (uparea ** b on those cells — evaluated by
 * the caller in the reference's dtype), elevtn PFD_F32 / PFD_F64; out int8: 1 floodplain, 0 not, -1 off the sequence. */
int pfd_floodplains(pfd_raster *h, int elev_dtype, const void *elevtn, const uint8_t *is_stream, const float *stream_h,
                    int8_t *out, int memspace);

/* core.snap in downstream direction, cell units (reference pyflwdir/core.py:440-480, Flwdir.snap
 * flwdir.py:404-463; used by basins(streams=...) / add_pits(streams=...), flwdir.py:805-811): per start cell
 * (k HOST indices) the first cell downstream, itself included, where mask != 0, or the pit its path ends in;
 * dist_out = cells walked (float32 like the reference); max_hops < 0: unlimited.  64-bit cell indices: both snap
 * entries serve whole rasters of any size. */
int pfd_snap_downstream(pfd_raster *h, const int64_t *idxs, int64_t k, const uint8_t *mask, int memspace,
                        int64_t max_hops, int64_t *idxs_out, float *dist_out);
/* The general form of core.snap (reference pyflwdir/core.py:440-480, core._trace :308-366, Flwdir.snap
 * flwdir.py:500-560): `idxs_us_main` == NULL walks downstream, else upstream along the caller's main upstream
 * cells (HOST, n int64, negative = none); `step_lengths` == NULL counts cells, else adds metres from the HOST
 * table [2*nrow - 1][3] float64 (row + next row; vertical, horizontal, diagonal step: gis_utils.distance
 * evaluated by the host); `mask` (HOST, nullable) ends a walk on the first cell where it is set; with
 * has_max_length a walk also ends before the step that would exceed max_length.  Distances accumulate in float64
 * (the reference's Python float) and are stored as float32. */
int pfd_snap(pfd_raster *h, const int64_t *idxs, int64_t k, const uint8_t *mask, const int64_t *idxs_us_main,
             const double *step_lengths, int has_max_length, double max_length, int64_t *idxs_out, float *dist_out);

/* ---- instrumentation ---------------------------------------------------------------------
 * HIP-event timing (events recorded on the handle's own stream) of the phases of the LAST
 * sweep/ordering call on the handle.  Enable with pfd_set_profiling(h, 1).  Up to max_seg
 * segments are returned: ms[i] GPU milliseconds, launches[i] kernel launches in the segment,
 * names = segment names joined by ';' (e.g. "order_cells;init;sweep_count_up").  enable = 2 additionally makes
 * the tile passes of upstream_area("cell") count their pointer-doubling rounds (pfd_graph_stats; costs two
 * atomics per tile, so not for timed runs). */
int pfd_set_profiling(pfd_raster *h, int enable);
int pfd_last_timing(pfd_raster *h, int max_seg, double *ms, int64_t *launches, char *names,
                    size_t names_len, int *nseg);

/* Graph statistics a benchmark reports next to every number: stats[0] = n_valid,
 * [1] = n_pits, [2] = max rank = longest flow path in cells (reference core.rank, pyflwdir/core.py:17-47;
 * -1 if the raster holds cycles or is a row block, -2 if it is beyond the slot ids of the tiled rank query: unknown), [3..11] = number of valid cells with 0..8
 * upstream cells (reference core.upstream_count, pyflwdir/core.py:50-61); [12..15] = pointer-doubling rounds
 * of the last upstream_area("cell") pass this handle ran under pfd_set_profiling(h, 2): max and sum over the tiles of the
 * local pass, max and sum of the final pass (0 if there was none).  Works on rasters beyond 2^32 cells. */
int pfd_graph_stats(pfd_raster *h, int64_t stats[16]);

/* Verifies an upstream_area("cell") result of this raster by its local equations, at any size
 * (whole rasters, incl. beyond 2^32 cells): res[0] = valid cells with upa != 1 + sum over the cells
 * draining into them, [1] = nodata cells != -9999, [2] = sum of upa over the pits, [3] = pits,
 * [4] = sum of all n values (two's complement), [5] = valid cells.  On a raster without cycles
 * res[0] == res[1] == 0 holds for exactly one array: the reference's result (streams.accuflux over
 * ones, pyflwdir/streams.py:15-41; invariant [2] == [5]: tests/test_streams_basins.py:24-27). */
int pfd_verify_upstream_area_cell(pfd_raster *h, const int32_t *upa, int memspace, int64_t res[8]);

/* The same for a basins() result with uint32 ids (reference pyflwdir/basins.py:12-18, core.py:120-146) and for a HAND
 * result (dem.py:299-330), each cell against its downstream cell only: res[0] = valid cells violating their equation
 * (labels: seeded cell == its id, other cells == the label of their downstream cell, 0 for a pit; HAND: 0 on drain
 * cells, else hand[ds] + (double)(elevtn[x] - elevtn[ds]) with the difference in the elevation dtype, bit for bit),
 * res[1] = nodata cells != 0 / != -9999, res[2] = sum of all values (HAND: of their bit patterns), res[3] = labelled
 * cells / drain cells.  `outlets` (k distinct linear indices, HOST) and `ids` (HOST) are the seeds of the labels. */
int pfd_verify_basins(pfd_raster *h, const int64_t *outlets, const uint32_t *ids, int64_t k, const uint32_t *labels,
                      int memspace, int64_t res[4]);
int pfd_verify_hand(pfd_raster *h, const uint8_t *drain, int elev_dtype, const void *elevtn, const double *hand,
                    int memspace, int64_t res[4]);

/* sum of n int32 values in HBM (two's complement, 64 bit): the checksum multi-block runs compare with a
 * single-GPU run of the same raster */
int pfd_checksum_i32(int device, const int32_t *dev_ptr, int64_t n, int64_t *sum);
/* number of NaN / +-inf values of a DEVICE array (dtype PFD_F32 or PFD_F64): callers with device-resident elevations check
 * them with it before the row-block HAND (pfd_hand_block), whose "-inf = height not known yet" a non-finite difference imitates */
int pfd_count_nonfinite(int device, int dtype, const void *dev_ptr, int64_t n, int64_t *count);

/* ---- elementwise: the small expressions between two sweeps, on arrays that stay in HBM (csrc/elementwise.hip) ---------
 * What a front end computes with numpy between two calls (`drain == 1`, `mask != 0`, `upa > t`, an int -> float64
 * widening) for per-cell arrays that never leave the device.  No handle: `device` is the GPU, every pointer is a DEVICE
 * pointer to n elements (n >= 0; n may exceed 2^32), `out` never aliases an input.  Element dtypes: PFD_U8 (also bool:
 * bytes 0 / 1), PFD_I8, PFD_I32, PFD_U32, PFD_I64, PFD_F32, PFD_F64; any other code is PFD_EUNSUPPORTED.  Scalars travel
 * as the pair scalar_i (integer dtypes) / scalar_f (float dtypes; rounded to float for PFD_F32), like nodata_i / nodata_f.
 * Ordering: see "memory spaces" — every call waits for its kernels before it returns.
 * pfd_ew_compare — out[i] = 1 if the relation holds between a[i] and the scalar, else 0.  `rel` is a set of outcomes, the
 *   sum of PFD_EW_LT (a < s), PFD_EW_EQ, PFD_EW_GT and PFD_EW_UNORDERED (one side is NaN): < is 1, <= 3, > 4, >= 6, == 2,
 *   != 13 — IEEE comparisons: NaN gives 0 except for !=, -0.0 == 0.0.  compare_dtype == dtype compares in the array's own
 *   type; compare_dtype == PFD_F64 converts every element to double first (round to nearest, as a C cast does) and
 *   compares with scalar_f: what numpy does for an integer or float32 array and a float64 scalar.
 * pfd_ew_logic — byte masks holding 0 / 1: PFD_EW_AND / PFD_EW_OR / PFD_EW_XOR of a and b, PFD_EW_NOT of a (b ignored).
 * pfd_ew_where — out[i] = mask[i] != 0 ? a[i] : b[i], or the scalar in place of b[i] when b is NULL; a, b and out of `dtype`.
 * pfd_ew_convert — the conversions that are exact for every value: PFD_U8 / PFD_I8 -> PFD_I32; PFD_I32 / PFD_U32 ->
 *   PFD_I64 / PFD_F64; PFD_F32 -> PFD_F64.  Anything else is PFD_EUNSUPPORTED.
 * pfd_ew_reduce — reductions with one answer whatever the execution order: PFD_EW_COUNT the number of elements != 0 (a NaN
 *   counts) in *res_i; PFD_EW_MIN / PFD_EW_MAX the smallest / largest element, integer dtypes in *res_i, float dtypes in
 *   *res_f (as a double; -0.0 orders below 0.0), with *has_nan = 1 when a float array holds a NaN — *res_f is then the
 *   extreme of the other elements and the caller answers NaN, as np.min / np.max do.  n == 0: PFD_EINVAL for MIN / MAX.
 *   Two launches (a partial per workgroup, then one workgroup over the partials), no atomics, no float arithmetic. */
#define PFD_EW_LT 1
#define PFD_EW_EQ 2
#define PFD_EW_GT 4
#define PFD_EW_UNORDERED 8
#define PFD_EW_AND 0
#define PFD_EW_OR 1
#define PFD_EW_XOR 2
#define PFD_EW_NOT 3
#define PFD_EW_COUNT 0
#define PFD_EW_MIN 1
#define PFD_EW_MAX 2
int pfd_ew_compare(int device, int rel, int dtype, const void *a, int compare_dtype, int64_t scalar_i, double scalar_f,
                   uint8_t *out, int64_t n);
int pfd_ew_logic(int device, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, int64_t n);
int pfd_ew_where(int device, int dtype, const uint8_t *mask, const void *a, const void *b, int64_t scalar_i, double scalar_f,
                 void *out, int64_t n);
int pfd_ew_convert(int device, int src_dtype, const void *a, int dst_dtype, void *out, int64_t n);
int pfd_ew_reduce(int device, int op, int dtype, const void *a, int64_t n, int64_t *res_i, double *res_f, int *has_nan);

/* ---- synthetic rasters (bench / tests; device twin of oracle/pfd_oracle.c orc_synth_*) ---- */
/* writes rows [row0, row0+nrows) of the nrow x ncol synthetic raster to device memory */
int pfd_synth_d8(int device, uint64_t seed, int64_t nrow, int64_t ncol, int64_t tilt, int64_t white,
                 int32_t nodata_pct, int64_t row0, int64_t nrows, uint8_t *out_dev);
int pfd_synth_elev_f32(int device, uint64_t seed, int64_t nrow, int64_t ncol, int64_t tilt,
                       int64_t white, int32_t nodata_pct, int64_t row0, int64_t nrows, float *out_dev);
/* a host base raster (brow x bcol D8 codes) tiled over nrow x ncol cells in HBM, every copy inside a one-cell nodata
 * frame: bench.py's realistic regime (the reference's Rhine sub-basin) at sizes that are never shipped over PCIe */
int pfd_synth_mosaic(int device, const uint8_t *base_host, int64_t brow, int64_t bcol, int64_t nrow, int64_t ncol,
                     uint8_t *out_dev);
/* measurement aid: one streaming pass over nbytes of buf_dev with `width`-byte accesses per lane (1, 4, 8, 16), reading or
 * writing — a kernel with a known byte count, for calibrating the rocprofv3 FETCH_SIZE / WRITE_SIZE counters per access
 * width (tools/prof_calib.sh) */
int pfd_calib_traffic(int device, void *buf_dev, size_t nbytes, int width, int write);
int pfd_synth_weights_f32(int device, uint64_t seed, int64_t i0, int64_t n, float *out_dev);

#ifdef __cplusplus
}
#endif
#endif /* PFD_H_ */
