// How a scan gets onto the device, behind the C ABI (pk_filter.hpp): the pinned staging ring and the device block, the host half of
// the maximum-likelihood upload (stage_ml_scan; the block's layout and fill are pk_scan_block.hpp's), the known-ids block, what the
// scan-taking calls check of their arguments, the ids read-out, and pk_stage_scan.  Host orchestration only.
#include "pk_filter.hpp"

static int ensure_scan_capacity(pk_filter* f, size_t bytes) {
  if (bytes <= f->scan_cap) return PK_OK;
  int rc;
  if ((rc = dev_reserve(f, &f->scan_dev, &f->scan_cap, bytes, bytes + bytes / 4 + 4096))) return rc;
  f->gmax_fused = false;  // the running-max keys lived in the block that was just freed
  return PK_OK;
}

int ensure_ids_capacity(pk_filter* f, int B) {
  const int64_t need = f->d.P * (int64_t)B;
  return dev_reserve(f, &f->ids_dev, &f->ids_cap, need, need);
}

// An upload that reads staging slot `slot` has just been enqueued on the stream.
int note_upload(pk_filter* f, int slot) {
  f->slot_seq[slot] = ++f->upload_seq;
  if ((slot & 3) == 3) {  // an event record costs the stream a few microseconds: one per four uploads
    PK_HIP(hipEventRecord(f->stage_done[slot], f->stream));
    f->event_seq[slot] = f->upload_seq;
  }
  return PK_OK;
}

// One scan block, staged in slot `slot`, host -> device in stream order.  The staging ring is pinned and device-mapped, so a small
// kernel reads it directly (k_upload); sizes are padded to 16 bytes on both sides.  The copy engine where the mapping is not available.
int upload_scan(pk_filter* f, const unsigned char* st, size_t bytes, int slot) {
  void* dev_view = nullptr;
  if (f->opt.upload_kernel && hipHostGetDevicePointer(&dev_view, const_cast<unsigned char*>(st), 0) == hipSuccess && dev_view) {
    launch_upload(f->stream, f->scan_dev, dev_view, bytes);
  } else {
    (void)hipGetLastError();
    PK_HIP(hipMemcpyAsync(f->scan_dev, st, bytes, hipMemcpyHostToDevice, f->stream));
  }
  return note_upload(f, slot);
}

// Next pinned staging block of at least `bytes` (waits for the upload that last read it), and a device block that holds as much.
int take_stage(pk_filter* f, size_t bytes, unsigned char** out, int* slot) {
  if (bytes > f->stage_cap) {
    PK_HIP(hipStreamSynchronize(f->stream));
    int rc;
    f->stage_cap = 0;
    size_t cap = bytes + bytes / 4 + 4096;
    for (int i = 0; i < pk_filter::kRing; ++i) {
      dev_free(f, &f->stage[i]);
      if ((rc = host_alloc(f, &f->stage[i], cap, hipHostMallocMapped))) return rc;
      if (!f->stage_done[i]) PK_HIP(hipEventCreateWithFlags(&f->stage_done[i], hipEventDisableTiming));
      f->slot_seq[i] = 0;  // the stream is idle: nothing reads the old blocks any more
    }
    f->stage_cap = cap;
  }
  int i = f->stage_next;
  f->stage_next = (i + 1) % pk_filter::kRing;
  // Slot i may still be read by upload number slot_seq[i]; any event recorded at or after that upload
  // covers it.  Normally that is the record behind slot (i | 3) of the previous trip round the ring;
  // when that slot's scan was discarded before its upload (pk_stage_scan followed by a supplied-ids
  // observe, an error between take_stage and the upload) no such record exists and one is made now.
  const uint64_t need = f->slot_seq[i];
  if (need != 0) {
    int ev = -1;
    for (int j = 0; j < pk_filter::kRing; ++j)
      if (f->event_seq[j] >= need && (ev < 0 || f->event_seq[j] < f->event_seq[ev])) ev = j;
    if (ev < 0) {
      PK_HIP(hipEventRecord(f->stage_done[i], f->stream));
      f->event_seq[i] = f->upload_seq;
      ev = i;
    }
    PK_HIP(hipEventSynchronize(f->stage_done[ev]));
    f->slot_seq[i] = 0;
  }
  *out = f->stage[i];
  *slot = i;
  return ensure_scan_capacity(f, bytes);
}

// Host half of the ML scan upload: the block is filled in a pinned staging slot (ml_scan_fill, ml_scan_ranges; no device work; may
// synchronise only to grow buffers).  Range rows travel only where some blob has a range (rs->any): else the bytes it always staged.
int stage_ml_scan(pk_filter* f, const double* blobs, int B, const RangeScan* rs) {
  int rc;
  if (B > 65535) return fail(PK_ERR_UNSUPPORTED, "maximum-likelihood association handles at most 65535 blobs per scan (got %d)", B);
  // the general EKF kernel (every ML route's last resort) builds per-particle chains in LDS
  if (observe_general_lds_bytes(f->d.lay.Lp, B) > kMaxDynLds)
    return fail(PK_ERR_UNSUPPORTED,
                "maximum-likelihood association: %d landmarks + 2 x %d blobs need %zu bytes of LDS chains per particle, the "
                "workgroup has %zu", f->d.lay.Lp, B, observe_general_lds_bytes(f->d.lay.Lp, B), (size_t)kMaxDynLds);
  if ((rc = ensure_ids_capacity(f, B))) return rc;
  pk_filter::Staged& sg = f->staged;
  sg.valid = false;
  sg.uploaded = false;
  sg.with_ranges = rs && rs->armed;
  sg.ranged = rs && rs->any;
  if ((rc = take_stage(f, ml_scan_worst_bytes(B, sg.ranged), &sg.st, &sg.slot))) return rc;
  // the grid kernel keeps landmark indices as u16 and its tables in LDS: duplicated column lists when they fit (48 B a blob), else the 9-range walk
  sg.use_grid = f->opt.assoc_kernel == 0 && f->d.lay.L <= 65535;
  const bool dup = f->opt.assoc_dup && assoc_grid_lds_bytes(kGridMax * kGridMax * kGridMax, B, 9 * B + 16) <= kMaxDynLds;
  ml_scan_fill(sg.st, blobs, B, sg.use_grid, dup, &sg.g, &sg.n9);
  if (sg.use_grid && assoc_grid_lds_bytes(sg.g.ncell, B, sg.n9) > kMaxDynLds) sg.use_grid = false;  // scan too large for LDS tables
  sg.lay = ml_scan_ranges(sg.st, B, sg.use_grid, sg.g.ncell, sg.n9, sg.ranged ? rs->rv.data() : nullptr);
  sg.B = B;
  sg.valid = true;
  return PK_OK;
}

int upload_known_scan(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, bool with_ids, KnownScan* out, const RangeScan* rs) {
  int rc;
  const MapLayout& lay = f->d.lay;
  KnownScan k;
  k.lay = known_scan_layout(B, lay.Lp, with_ids, rs && rs->any);
  unsigned char* st = nullptr;
  int slot = 0;
  if ((rc = take_stage(f, k.lay.upload_bytes, &st, &slot))) return rc;
  memset(st, 0, kCtlBytes);
  if (B > 0) memcpy(st + k.lay.blobs, blobs, (size_t)B * 4 * sizeof(double));
  if (with_ids && B > 0) memcpy(st + k.lay.ids, ids, (size_t)B * sizeof(int32_t));
  if (k.lay.rng) memcpy(st + k.lay.rng, rs->rv.data(), (size_t)B * 2 * sizeof(double));
  int32_t* first = reinterpret_cast<int32_t*>(st + k.lay.first);
  int32_t* next = reinterpret_cast<int32_t*>(st + k.lay.next);
  std::vector<int32_t> last((size_t)lay.Lp, -1);
  for (int l = 0; l < lay.Lp; ++l) first[l] = -1;
  for (int b = 0; b < B; ++b) {
    next[b] = -1;
    int id = ids[b];
    if (id == 0) {
      ++k.n_unmatched;
      continue;
    }
    if (first[id - 1] < 0) {
      first[id - 1] = b;
    } else {
      next[last[id - 1]] = b;
      k.single_sightings = false;
    }
    last[id - 1] = b;
  }
  if ((rc = upload_scan(f, st, k.lay.upload_bytes, slot))) return rc;
  *out = k;
  return PK_OK;
}
// ... and the device views of that block: a scan with supplied ids has B and the blobs alone
ScanTables known_scan_tables(const pk_filter* f, const KnownScan& ks, int B) {
  ScanTables scan;
  scan.B = B;
  scan.blobs = reinterpret_cast<const double*>(f->scan_dev + ks.lay.blobs);
  return scan;
}
KnownChains known_chains(const pk_filter* f, const KnownScan& ks) {
  KnownChains c;
  c.first = reinterpret_cast<const int32_t*>(f->scan_dev + ks.lay.first);
  c.next = reinterpret_cast<const int32_t*>(f->scan_dev + ks.lay.next);
  c.n_unmatched = ks.n_unmatched;
  return c;
}

int check_scan_shape(const pk_filter* f, const char* who, const double* blobs, int32_t B) {
  if (B < 0 || (B > 0 && !blobs)) return fail(PK_ERR_INVALID, "%s: bad blobs", who);
  if (!f->map_loaded) return fail(PK_ERR_STATE, "%s: no map uploaded (pk_upload_map)", who);
  return PK_OK;
}
int check_scan_values(const pk_filter* f, const char* who, const double* blobs, int32_t B, const int32_t** ids) {
  for (int i = 0; i < 4 * B; ++i)
    if (!std::isfinite(blobs[i])) return fail(PK_ERR_INVALID, "%s: blob %d is not finite", who, i / 4);
  if (!ids) return PK_OK;
  static const int32_t no_ids = 0;
  if (!*ids && B == 0) *ids = &no_ids;
  if (*ids)
    for (int b = 0; b < B; ++b)
      if ((*ids)[b] < 0 || (*ids)[b] > f->d.lay.L) return fail(PK_ERR_INVALID, "%s: ids[%d] = %d outside 0..%d", who, b, (*ids)[b], f->d.lay.L);
  return PK_OK;
}
int refuse_grow_ids(const char* who) {
  return fail(PK_ERR_STATE, "%s: the new-landmark bookkeeping (pk_grow_enable) follows the maximum-likelihood association: no ids", who);
}

int return_ids(pk_filter* f, int32_t* ids_out, int32_t B, const int32_t* supplied) {
  if (!ids_out || B <= 0) return PK_OK;
  if (supplied) {
    for (int64_t p = 0; p < f->d.P; ++p) memcpy(ids_out + (size_t)p * B, supplied, (size_t)B * 4);
    return PK_OK;
  }
  PK_HIP(hipMemcpyAsync(ids_out, f->ids_dev, (size_t)f->d.P * B * 4, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

extern "C" int pk_stage_scan(pk_filter* f, const double* blobs, int32_t B) {
  if (!f) return fail(PK_ERR_INVALID, "pk_stage_scan: NULL handle");
  RangeScan rs;
  int rc;
  if ((rc = ranges_take(f, "pk_stage_scan", B, &rs))) return rc;
  if (B < 1 || !blobs) return fail(PK_ERR_INVALID, "pk_stage_scan: needs at least one blob");
  if ((rc = check_scan_shape(f, "pk_stage_scan", blobs, B))) return rc;
  if ((rc = check_scan_values(f, "pk_stage_scan", blobs, B))) return rc;
  if ((rc = use_device(f))) return rc;
  if (f->dense) {  // no tables to build: the blobs wait on the host
    f->dense_staged.assign(blobs, blobs + 4 * (size_t)B);
    return PK_OK;
  }
  f->dense_staged.clear();
  return stage_ml_scan(f, blobs, B, &rs);
}
