// K2 + K3 in ONE pass with the settling of contested blobs turned into a STATIC publish / subscribe through LDS:
// k_step_pub (512 < L <= 2048), and k_cand_entries, which lays the publish table out once per scan.
//
// Hand-written gfx950 (CDNA4, wave64) kernels of the FastSLAM particle update; see DESIGN.md section 4.
// No MFMA: the algebra is 2x2 / 3x3 and register resident (pk_math.hpp).
//
// What couples the landmarks of a particle in maximum-likelihood association (prkt_core_v2.py:353-381) is a blob that
// passes the gates of several landmarks: it goes to the most probable one, the earliest on a tie (:377), to nobody when
// every probability is 0 (:369).  k_step_regs settles that with per-blob counters, a probability queue, bids and eight
// workgroup barriers per particle -- one particle per CU in lock step.  Here WHO can contend for a blob is known before
// the particle is looked at: the reference particle's candidate lists (k_candidates), landmark -> blobs and blob ->
// landmarks.  So every (landmark, blob) pair that can be contested owns a fixed 8-byte entry of an LDS table for the
// whole scan (blob t: entries offs[t] .. offs[t] + n[t] - 1, one per landmark of its inverse list, ascending):
//   publish    the landmark's lane writes its verdict there -- +inf when the blob does not pass its gates or has
//              probability 0, else the pair's KEY = -2 log(probability) up to rounding --
//   barrier A
//   settle     one lane per contested blob reads the blob's run of entries in one batch: the smallest key takes the
//              blob, the lowest landmark on equal keys; the winner's entry is overwritten with the marker -inf
//   barrier B
//   subscribe  every landmark's lane reads the entries of the blobs it passes: the marker means "yours"
//   barrier C  (hands the table to the next particle).
// No atomics, no queue, three barriers per particle that stand close together (k_step_regs: eight), and between C and the
// next A the long phases -- rows arriving, gates, keys, EKF updates, stores -- run without any synchronisation, so the waves
// of a workgroup drift apart and one wave's memory time is another's arithmetic.  (A first version let every landmark's
// lane read its rivals' entries itself, one after the other: 40 % of the kernel's time went into those dependent LDS reads.)
//
// Keys instead of probabilities: the reference compares pr = (500 exp(-a2/2)) (500 exp(-a3/2)) / 250000 (:439-455);
// -2 log pr = a2 + a3 orders the same way wherever the two differ by more than rounding.  The kernel therefore FLAGS a
// particle for the general kernels (exact probabilities, as before) whenever keys of two contenders are closer than 1e-7
// without being identical (identical landmarks give identical keys: a tie, :377), and wherever pr would be subnormal
// (keys beyond 1350) with a second contender; whether pr is > 0 at all (:369, strict) is decided from the keys with
// margins on both sides of the float64 underflow edge (keys 1489 ... 1491.5) and evaluated exactly inside them.
//
// Shape: persistent 512-lane workgroups, one per CU, FOUR landmarks per lane (two adjacent pairs, 16-byte row accesses),
// the particle's whole map in registers from its single coalesced load to its single coalesced store; 8 waves x 256
// VGPRs are the CU's register file, and 256 registers hold a lane's four landmarks (116) plus the update's working set
// without parking anything in LDS.
//
// Round 4: the lanes take their landmarks through a per-scan ORDER of sixteen-landmark groups (k_cand_entries
// ranks them by the blobs inside the reference particle's gates and by list length: a round of gates or verdicts costs the whole
// wave its arithmetic when one lane needs it); memory requests are issued in the order of their urgency (the texture addresser
// serves a CU's vector-memory instructions in order); landmarks that pass more blobs than they have slots are settled in the
// kernel.  k_step_pub_big (2 048 < L <= 6 144, two passes over the map, scan records in L2): the gates' first look goes to a float
// copy of a candidate's bearing and colour, look-alikes beyond the underflow edge take no slot, the publish table is rank-major.
#include <type_traits>

#include "pk_colour.hpp"
#include "pk_device.hpp"
#include "pk_launch.hpp"
#include "pk_pub_math.hpp"
#include "pk_pub_layout.hpp"

namespace pk {

// Diagnostic builds only (python -m parakeet_slam_amd.build --variant NAME -DPK_PUB_ABLATE=n, never shipped): phases left out
// from the back -- 1 no EKF updates, 2 nor subscribe, 3 nor verdicts, 4 nor gates (rows in, barriers, rows out) -- to see
// what each costs in place.  Results are wrong by construction.
#ifndef PK_PUB_ABLATE
#define PK_PUB_ABLATE 0
#endif

typedef double Double2 __attribute__((ext_vector_type(2)));
typedef int Int2 __attribute__((ext_vector_type(2)));

// A particle's pose component / source slot through the constant address space: uniform reads become scalar loads (their
// own counter, the scalar cache) instead of vector loads that queue behind the rows in flight.  The poses are not written
// while the kernel runs; src[p] is written only by the workgroup that owns particle p, after it has read it.
__device__ __forceinline__ double pose_scalar(const double* a, int64_t p) {
  return ((const __attribute__((address_space(4))) double*)a)[p];
}
__device__ __forceinline__ int32_t regs_source_pub(const int32_t* src, int64_t p) {
  return ((const __attribute__((address_space(4))) int32_t*)src)[p];
}

struct PubArgs {
  SlotSource ss;
  unsigned char* map_dst;
  size_t count_off;
  int32_t* src;
  const double *x, *y, *h;
  double* logw;
  const double* exact;          // [B][6] cell order: bearing, r, g, b, ux, uy
  const unsigned short* order;  // [B] cell order -> scan order
  const unsigned char* immutable;
  const uint4* cand;            // [Lp][2]: reference (eb, r, g, b as float) | 8 x u16 blobs
  const uint4* erec;            // [Lp]: 8 x u16 publish entries of those blobs (0xFFFF: nobody else lists the blob)
  const unsigned* glist;        // [B + 1]: the blobs at least two landmarks list: first entry | contenders << 16; [B]: how many
  const unsigned* skip;         // != 0: this scan is not ours (a list overflowed, or the table does not fit)
  const float4* gate4;          // [B] k_step_pub_big: bearing, r, g, b as float (NaN: out of the range the margins cover), else null
  const uint4* far;             // [Lp + spare][1 + slots / 8]: (Kb, Ib, n, 0) | the far list of every landmark (k_candidates), or null
  unsigned char* pflag_out;     // [P] 1 = general route
  unsigned* n_flagged;
  int64_t P, p_begin;
  int L, Lp, B;
  int ecap;                     // entries of the publish table in LDS
  int reset;
  int lean = 0;                 // k_step_pub<2, 512> only: != 0: the (wave, pair) groups k_cand_entries marked lean take the lean body
                                //   (pub_lean_pair); pairs of theirs that fall back to the usual body are counted in stats[6]
  unsigned long long* gmax_key;
  Noise<double> qt;
  // (k_step_pub_duo only; behind everything the other kernels read)
  const unsigned* stats;        // [7] k_cand_entries' figures of this scan: [0] the entries of its publish table, [3] its longest list
  int tbytes;                   // bytes of LDS the publish table and the overflow area share
  const uint4* prim;            // the two-pass kernels: every landmark's primary blob in landmark order (prim_table_uint4), or null
  const double* ctab = nullptr; // table mode (k_step_pub<NP, 512, true>; pk_colour.hpp): the colour table [depth][6][Lp], else null
  unsigned* ctab_max = nullptr; //   out: the highest level a lane read (one atomic per workgroup)
  int ctab_depth = 0;
  unsigned* unm;                // growing maps (section 8(f4)): out [P][unm_words], bit b of a particle's row = blob b (SCAN order) is matched by
  int unm_words;                //   none of its landmarks (:92-95: k_new_landmarks takes those through add_hypothesis), or null
};

// Growing maps on the one-pass routes (round 6; VERDICT round 5, missing #2): the new-landmark bookkeeping (pk_k_grow.hip,
// prkt_core_v2.py:92-95, :546-746) wants the blobs a particle matched to NO landmark.  Until now it read them off the ids the general
// association kernel leaves in HBM, so a growing filter took the general route (an O(P B L) association kernel plus an ids round trip:
// 58 GB per step at 100 000 x 2 000 against 36-40 for the one-pass kernel).  The publish / subscribe kernels know those blobs behind
// barrier A -- any[t] == 0: the same test that adds log 0.1 per unseen blob (:94-95) -- and leave them as a bit row per particle, in
// SCAN order (k_new_landmarks takes them in that order: each sees what the ones before it stored).  kPubUnmWords: the row's capacity.
constexpr int kPubUnmWords = 176;  // 5 632 blobs
template <int THREADS>
__device__ __forceinline__ void pub_note_unmatched(int tid, const unsigned char* anyc, const unsigned short* order, int B, unsigned Bp, unsigned* ubits) {
  for (unsigned w = (unsigned)tid; w < Bp / 4u; w += THREADS) {
    const unsigned v = reinterpret_cast<const unsigned*>(anyc)[w];
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if ((int)(4 * w + b) < B && ((v >> (8 * b)) & 0xFFu) == 0u) {  // (a handful of blobs per particle, if any)
        const unsigned o = order[4 * w + b];
        atomicOr(&ubits[o >> 5], 1u << (o & 31u));
      }
  }
}
// ... behind barrier B: the row out, the LDS words cleared for the next particle (whose blobs are noted behind ITS barrier A)
template <int THREADS>
__device__ __forceinline__ void pub_store_unmatched(int tid, unsigned* ubits, unsigned* row, int words) {
  for (int w = tid; w < words; w += THREADS) {
    row[w] = ubits[w];
    ubits[w] = 0u;
  }
}

// The PRIMARY blob of a landmark -- the front of its candidate list: k_cand_entries puts the candidate closest in colour there -- has
// its records in a table in LANDMARK order (pk_kernels.hpp: prim_table_uint4).  Wherever every lane of a wave wants exactly that blob
// (the gates' first candidate: always; the verdicts' first slot, the blob the update applies: nearly always) the two-pass kernels
// read the table -- neighbouring lanes, neighbouring addresses -- instead of gathering the scan's records blob by blob, a cache line
// a lane.  Same bytes either way (k_cand_entries copies them), so the same results bit for bit.
struct PubPrim {
  const uint4* tab;  // the table (uniform)
  size_t Lpp;        // landmarks + spare records: the planes' stride (uniform)
  int lc;            // the lane's first landmark (landmark j of the lane: lc + j)
  // (addresses are made where they are used: held as three per-lane pointers from the gates to the verdicts they cost six VGPRs)
  __device__ __forceinline__ double2 z01(int j) const { return reinterpret_cast<const double2*>(tab + Lpp)[lc + j]; }      // exact bearing, r
  __device__ __forceinline__ double2 z23(int j) const { return reinterpret_cast<const double2*>(tab + 2 * Lpp)[lc + j]; }  // exact g, b
  __device__ __forceinline__ double2 dir(int j) const { return reinterpret_cast<const double2*>(tab + 3 * Lpp)[lc + j]; }  // ray direction
  __device__ __forceinline__ unsigned t0(int j) const { return reinterpret_cast<const unsigned*>(tab + 4 * Lpp)[lc + j]; }  // the blob (0xFFFF: none)
};

// dynamic LDS: exact records 48 B | publish table 8 (ecap + 2: a dump entry, padding) | binfo 4 B | order 2 B |
// any 2 x (B + 16: a dump byte) (B padded to 16) | the landmarks' immutable flags, 1 B each (kPubImmBytes)
constexpr size_t kPubImmBytes = 2048;  // k_step_pub: maps up to 2 048 landmarks
// ... | the landmarks' far bounds (Kb, Ib as float, 8 B each: pk_pub_math.hpp) -- 2 048 landmarks, 512 for the 256-lane instance
__host__ __device__ inline size_t pub_bound_lds_bytes(bool small) { return (small ? 512 : 2048) * 8; }
__host__ __device__ inline size_t pub_fixed_lds_bytes(int B, bool small = false) {
  const size_t Bp = ((size_t)B + 15) & ~(size_t)15;
  return Bp * 48 + 16 + Bp * 4 + Bp * 2 + 2 * (Bp + 16) + kPubImmBytes + pub_bound_lds_bytes(small);
}
size_t step_pub_lds_bytes(int B, int ecap, bool small) { return pub_fixed_lds_bytes(B, small) + (size_t)ecap * 8; }  // (the 16 spare bytes: the dump entry)
int step_pub_entry_capacity(int B) {
  const size_t fixed = pub_fixed_lds_bytes(B);
  if (fixed + 64 * 8 > kMaxDynLds) return 0;
  const size_t e = (kMaxDynLds - fixed) / 8;
  return (int)(e > 65534 ? 65534 : e);
}

int step_pub_entry_capacity_small(int B) {
  const size_t budget = 52 * 1024, fixed = pub_fixed_lds_bytes(B, true);  // three workgroups per CU
  if (fixed + 64 * 8 > budget) return 0;
  return (int)((budget - fixed) / 8);
}

// ------------------------------------------------------------------ per-landmark pieces of k_step_pub
// Control flow is kept WAVE-UNIFORM wherever it can be: loops end on a ballot, bodies are predicated, the entries a lane has
// nothing to say about go to a dump entry of the table -- a divergent branch costs a handful of scalar instructions, and a
// first version that branched per candidate and per slot issued as many scalar as vector instructions.
//
// What a lane keeps about one landmark's (<= 4) gate-passing blobs between the phases: per slot blob | entry << 16
// (0xFFFF: none / no other landmark lists the blob), most recent first, empty slots at the back.
template <int SL>
struct PubSlotsT {
  unsigned s[SL];
  unsigned st;  // 4 bits per slot: 1 probability > 0, 4 take
};
using PubSlots = PubSlotsT<kPubSlots>;
constexpr PubSlots kPubNoSlots = {{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, 0u};
template <int SL>
__device__ __forceinline__ void pub_rotate(PubSlotsT<SL>& q) {  // slot 0 goes to the back, its state bits with it
  const unsigned w = q.s[0];
#pragma unroll
  for (int k = 0; k + 1 < SL; ++k) q.s[k] = q.s[k + 1];
  q.s[SL - 1] = w;
  if constexpr (SL == 8) {
    q.st = (q.st >> 4) | (q.st << 28);
  } else {  // (the bits above the slots' stay where they are: pub_gatesN<OVF> keeps the landmark's pass mask there)
    const unsigned lowmask = (1u << (4 * SL)) - 1u, low = q.st & lowmask;
    q.st = (((low >> 4) | (low << (4 * SL - 4))) & lowmask) | (q.st & ~lowmask);
  }
}

__device__ __forceinline__ double pub_inf() { return __longlong_as_double(0x7FF0000000000000ll); }

// Gates (prkt_core_v2.py:433, :441) of the TWO landmarks of a pair against their candidate lists: as regs_gates_cand, the
// records read from the LDS copy of the scan, two candidates of each landmark per round (four independent chains: with two
// waves per SIMD the instruction stream itself has to cover the arithmetic and LDS latencies); candidates that fail are
// published as "not a contender" on the spot (a passing one's entry is overwritten by pub_keys).  dump: the table's spare
// entry.  has: the landmark exists (lanes beyond the map carry empty lists).
struct PubGateIn {
  uint4 ref;
  uint4 cw[2], ew[2];  // the candidate blobs and their publish entries, 16 bits each ([1] only with sixteen-entry lists)
  double mx, my, mr, mg, mb;
  bool has;
  double fk, fi;  // GT only: where fi > 0 the landmark's keys are at least fk + fi |colour difference|^2 (pub_far_bound)
};
// N: landmarks worked on side by side; W4: uint4 words per list (1: eight candidates, 2: sixteen)
// OVF: a landmark may pass MORE blobs than it has slots without the particle being flagged: bits 16.. of its slots' state word
// say which of its candidates passed, and pub_refill_slots brings in the ones the slots no longer hold (round 4: what flagged up to 13 % of the
// particles on some stretches of the bench's trajectory and sent them through the second-chance kernels).
// GT: the first look at a candidate goes to the float table gt (see k_cand_entries): certain either way for all but a candidate in
// a million, and only a wave with an uncertain one reads exact records (ex is global memory then, k_step_pub_big)
// PRIM (with GT): pga[pgi + j] = the float record of landmark j's FIRST candidate in the primary-blob table (plane 0, uniform base and
// the lane's first landmark: read where the gather it replaces stood, so that no register is held longer than before)
template <int N, int W4 = 1, int SL = kPubSlots, bool OVF = false, bool GT = false, bool PRIM = false>
__device__ __forceinline__ void pub_gatesN(PubSlotsT<SL> (&q)[N], double (&pse_out)[N], const PubGateIn (&in)[N], const double* ex,
                                           double* pub, unsigned dump, int* flag, double sx, double sy, double sh,
                                           const float4* gt = nullptr, const float4* pga = nullptr, int pgi = 0) {
  constexpr int NW = 4 * W4;  // 32-bit words per list, two candidates each
  double eb[N];
  bool inside[N];
  unsigned c[N][NW], e[N][NW];
  unsigned sl[N][SL];
  float dmin[N];  // colour distance of the blob in slot 0: the best colour match stands in front (pub_keys)
  int npass[N];
  unsigned pmask[N];  // OVF: bit k = candidate k of the list passed both gates
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double pse = pk_atan2(in[j].my - sy, in[j].mx - sx);
    pse_out[j] = pse;
    eb[j] = pse - sh;  // :408
    // (written so that a NaN anywhere breaks the margin)
    const double deb = eb[j] - (double)__uint_as_float(in[j].ref.x);  // 2 pi off: the other side of a branch cut, listed too (k_candidates)
    inside[j] = (fabs(deb) <= kCandBearing || fabs(deb - Consts<double>::two_pi) <= kCandBearing ||
                 fabs(deb + Consts<double>::two_pi) <= kCandBearing) &&
                fabs(in[j].mr - (double)__uint_as_float(in[j].ref.y)) <= kCandColour &&
                fabs(in[j].mg - (double)__uint_as_float(in[j].ref.z)) <= kCandColour &&
                fabs(in[j].mb - (double)__uint_as_float(in[j].ref.w)) <= kCandColour;
    // the list is filled from the front; a landmark beyond the map has none (its lane reads the table's spare records)
#pragma unroll
    for (int w = 0; w < W4; ++w) {
      c[j][4 * w + 0] = in[j].cw[w].x;
      c[j][4 * w + 1] = in[j].cw[w].y;
      c[j][4 * w + 2] = in[j].cw[w].z;
      c[j][4 * w + 3] = in[j].cw[w].w;
      e[j][4 * w + 0] = in[j].ew[w].x;
      e[j][4 * w + 1] = in[j].ew[w].y;
      e[j][4 * w + 2] = in[j].ew[w].z;
      e[j][4 * w + 3] = in[j].ew[w].w;
    }
    c[j][0] = in[j].has ? c[j][0] : 0xFFFFFFFFu;  // (belt and braces: one conditional move)
#pragma unroll
    for (int k = 0; k < SL; ++k) sl[j][k] = 0xFFFFFFFFu;
    dmin[j] = 3.0e38f;
    npass[j] = 0;
    pmask[j] = 0u;
  }
  // GT: the float records of a round's candidates (a list that has ended reads record 0; asked for a round AHEAD: +1.7 %, six
  // registers spilled -- profiles/r04/ab_big_gate_records_a_round_ahead.log)
  float4 nfa[GT ? N : 1], nfb[GT ? N : 1];
  auto gate_request = [&](int kk) {
    if constexpr (GT) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const unsigned ta = c[j][kk] & 0xFFFFu, tb = c[j][kk] >> 16;
        if (PRIM && kk == 0)  // (the front of the list: its record came side by side with the neighbours')
          nfa[j] = pga[pgi + j];
        else
          nfa[j] = gt[ta != 0xFFFFu ? ta : 0u];
        nfb[j] = gt[tb != 0xFFFFu ? tb : 0u];
      }
    }
  };
#pragma unroll  // (written out: the list words are addressed statically -- shifted through the registers every round they cost 1.3 %)
  for (int k = 0; k < NW; ++k) {
    const int kk = k;
    unsigned call = c[0][kk];
#pragma unroll
    for (int j = 1; j < N; ++j) call &= c[j][kk];
    if (__ballot((call & 0xFFFFu) != 0xFFFFu) == 0ull) break;  // wave-uniform: every list is through
    float4 cfa[GT ? N : 1], cfb[GT ? N : 1];
    if constexpr (GT) {
      gate_request(kk);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        cfa[j] = nfa[j];
        cfb[j] = nfb[j];
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const unsigned ta = c[j][kk] & 0xFFFFu, tb = c[j][kk] >> 16;
      const unsigned ea = e[j][kk] & 0xFFFFu, eb2 = e[j][kk] >> 16;  // (0xFFFF where the blob is: k_cand_entries)
      const bool va = ta != 0xFFFFu, vb = tb != 0xFFFFu;
      double cda, cdb;
      bool pa, pb;
      if constexpr (GT) {
        // float values within 2^-24 relative of the record's: the bearing within 4.8e-7, a colour within 6e-5, the squared colour
        // distance -- components below 17.4 where it matters -- within 6.3e-3; beyond 300.01 the error grows more slowly than
        // the distance.  (The order of the slots follows the float distances: it decides nothing.)
        const float4 fa = cfa[j], fb = cfb[j];
        cda = color_distance2(in[j].mr, in[j].mg, in[j].mb, (double)fa.y, (double)fa.z, (double)fa.w);
        cdb = color_distance2(in[j].mr, in[j].mg, in[j].mb, (double)fb.y, (double)fb.z, (double)fb.w);
        const double dba = fabs((double)fa.x - eb[j]), dbb = fabs((double)fb.x - eb[j]);
        const bool out_a = dba > 0.5 + 1e-6 || cda > 300.01, in_a = dba < 0.5 - 1e-6 && cda < 299.99;  // NaN: neither
        const bool out_b = dbb > 0.5 + 1e-6 || cdb > 300.01, in_b = dbb < 0.5 - 1e-6 && cdb < 299.99;
        // A blob that passes the gates but whose key is CERTAINLY beyond the underflow edge (probability 0: what pub_keysN calls
        // far -- once a landmark's colour block has tightened, every look-alike's) is no contender and takes no slot: at several
        // thousand blobs each landmark passes a handful of those, and each cost the verdicts a round of gathers from L2
        // (27 % of the kernel's time, profiles/r04/stamps_k_step_pub_big_*).  The float distance is within 6.3e-3 of the exact one.
        const bool far_a = in[j].fi > 0.0 && in[j].fk + (cda - 0.01) * in[j].fi > 1492.0;  // NaN: false
        const bool far_b = in[j].fi > 0.0 && in[j].fk + (cdb - 0.01) * in[j].fi > 1492.0;
        pa = va && in_a && !far_a;
        pb = vb && in_b && !far_b;
        const bool ua = va && !out_a && !in_a, ub = vb && !out_b && !in_b;
#ifdef PK_DIAG_BIG_NO_EXACT  // diagnostic build only: the uncertain ones count as outside -- to show that the edge test bites
        if (false) {
#else
        if (__ballot(ua || ub) != 0ull) {  // wave-uniform, rare: the exact records of the uncertain ones
#endif
          const double* ra = ex + 6 * (ua ? ta : 0u);
          const double* rb = ex + 6 * (ub ? tb : 0u);
          const double2 a01 = *reinterpret_cast<const double2*>(ra);
          const double2 a23 = *reinterpret_cast<const double2*>(ra + 2);
          const double2 b01 = *reinterpret_cast<const double2*>(rb);
          const double2 b23 = *reinterpret_cast<const double2*>(rb + 2);
          const double xa = color_distance2(in[j].mr, in[j].mg, in[j].mb, a01.y, a23.x, a23.y);
          const double xb = color_distance2(in[j].mr, in[j].mg, in[j].mb, b01.y, b23.x, b23.y);
          pa = ua ? (!(fabs(a01.x - eb[j]) > 0.5) && !(fabs(xa) > 300.0)) : pa;
          pb = ub ? (!(fabs(b01.x - eb[j]) > 0.5) && !(fabs(xb) > 300.0)) : pb;
        }
      } else {
        const double* ra = ex + 6 * (va ? ta : 0u);
        const double* rb = ex + 6 * (vb ? tb : 0u);
        const double2 a01 = *reinterpret_cast<const double2*>(ra);
        const double2 a23 = *reinterpret_cast<const double2*>(ra + 2);
        const double2 b01 = *reinterpret_cast<const double2*>(rb);
        const double2 b23 = *reinterpret_cast<const double2*>(rb + 2);
        cda = color_distance2(in[j].mr, in[j].mg, in[j].mb, a01.y, a23.x, a23.y);
        cdb = color_distance2(in[j].mr, in[j].mg, in[j].mb, b01.y, b23.x, b23.y);
        pa = va && !(fabs(a01.x - eb[j]) > 0.5) && !(fabs(cda) > 300.0);
        pb = vb && !(fabs(b01.x - eb[j]) > 0.5) && !(fabs(cdb) > 300.0);
      }
      pub[(pa || ea == 0xFFFFu) ? dump : ea] = pub_inf();
      pub[(pb || eb2 == 0xFFFFu) ? dump : eb2] = pub_inf();
      const unsigned wa = ta | (ea << 16), wb = tb | (eb2 << 16);
      // a passing blob goes to the front when its colour is the closest so far, else behind the front one
      {
        const float d = (float)cda;
        const bool front = pa && d < dmin[j];
#pragma unroll
        for (int k = SL - 1; k >= 2; --k) sl[j][k] = pa ? sl[j][k - 1] : sl[j][k];
        sl[j][1] = pa ? (front ? sl[j][0] : wa) : sl[j][1];
        sl[j][0] = front ? wa : sl[j][0];
        dmin[j] = front ? d : dmin[j];
      }
      {
        const float d = (float)cdb;
        const bool front = pb && d < dmin[j];
#pragma unroll
        for (int k = SL - 1; k >= 2; --k) sl[j][k] = pb ? sl[j][k - 1] : sl[j][k];
        sl[j][1] = pb ? (front ? sl[j][0] : wb) : sl[j][1];
        sl[j][0] = front ? wb : sl[j][0];
        dmin[j] = front ? d : dmin[j];
      }
      if constexpr (OVF)
        pmask[j] |= (pa ? (1u << (2 * kk)) : 0u) | (pb ? (2u << (2 * kk)) : 0u);
      else
        npass[j] += (pa ? 1 : 0) + (pb ? 1 : 0);
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if constexpr (OVF) {
      if (in[j].has && !inside[j]) *flag = 1;
    } else {
      if (in[j].has && (!inside[j] || npass[j] > SL)) *flag = 1;
    }
#pragma unroll
    for (int k = 0; k < SL; ++k) q[j].s[k] = sl[j][k];
    q[j].st = OVF ? (pmask[j] << 16) : 0u;  // (OVF: the pass mask rides above the slots' state bits until pub_refill_slots)
  }
}

// Look-alikes taken off the lists once per scan (pk_pub_math.hpp; k_candidates): a landmark whose OWN far bound (fk, fi) is not at
// least the one its list was pruned with -- (Kb, Ib) -- cannot rely on "far for everybody" and looks at its FAR list itself: a
// blob there that passes its gates (:433, :441) and is not certainly far by the landmark's own bound sends the particle to the
// fall-back kernels.  Wave-uniform and rare (a particle that missed most of the updates the reference particle made to a landmark).
// far_row: the pair's far records [hdr | list] x 2; ex: the scan's exact records (LDS or global); has: the landmark exists.
template <int N, int W4 = 1, class FarRow>
__device__ __forceinline__ void pub_far_recheck(const bool (&viol)[N], const Landmark<double>* const (&lmp)[N], const double (&pse)[N],
                                                const double (&fk)[N], const double (&fi)[N], const FarRow& far_row_fn, const double* ex,
                                                double sh, int* flag) {
  bool any = false;
#pragma unroll
  for (int j = 0; j < N; ++j) any |= viol[j];
  if (__ballot(any) == 0ull) return;  // wave-uniform: the usual case
  const uint4* far_row = far_row_fn();
  if (far_row == nullptr) return;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (__ballot(viol[j]) == 0ull) continue;  // wave-uniform
    const Landmark<double>& lm = *lmp[j];
    const double eb = pse[j] - sh;  // :408
    const unsigned* fw = reinterpret_cast<const unsigned*>(far_row + (1 + W4) * j + 1);
#pragma unroll 1
    for (int w = 0; w < 4 * W4; ++w) {
      const unsigned cw = viol[j] ? fw[w] : 0xFFFFFFFFu;
      if (__ballot((cw & 0xFFFFu) != 0xFFFFu) == 0ull) break;  // wave-uniform: the lists are filled from the front
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const unsigned t = (cw >> (16 * half)) & 0xFFFFu;
        const bool valid = t != 0xFFFFu;
        const double* rec = ex + 6 * (valid ? t : 0u);
        const double2 z01 = *reinterpret_cast<const double2*>(rec);
        const double2 z23 = *reinterpret_cast<const double2*>(rec + 2);
        const double cd = color_distance2(lm.mr, lm.mg, lm.mb, z01.y, z23.x, z23.y);
        const bool pass = valid && !(fabs(z01.x - eb) > 0.5) && !(fabs(cd) > 300.0);
        const double d1 = z01.y - lm.mr, d2 = z23.x - lm.mg, d3 = z23.y - lm.mb;
        const bool farp = fi[j] > 0.0 && fk[j] + (d1 * d1 + d2 * d2 + d3 * d3) * fi[j] > kPubFarKey;  // (as in pub_keysN's rounds; NaN: false)
        bad |= pass && !farp;
      }
    }
  }
  if (bad) *flag = 1;
}


// LEAN groups (k_step_pub<2, 512>; DESIGN.md section 4, "lean groups").  k_cand_entries marks the (wave, pair) groups all of whose 128
// landmarks are SIMPLE: a pruned candidate list of at most one blob that no other landmark lists.  Such a landmark needs none of the
// publish / subscribe machinery -- no slots to insert into, no second candidate, no table entry to write or read, no settling to wait
// for: the blob is its own if it passes the gates with a probability > 0 -- and of the key only on which side of the underflow edge
// it lies: log det is bounded by the determinants' exponents (e ln 2 above, (e - 1) ln 2 below), which saves the logarithm.
// This body DECIDES only; every number that reaches the map or the weight is made by the same calls on the same arguments as ever
// (pk_atan2, ekf_update).  Whatever it cannot decide with certainty -- a key inside or near the edge strip, odd covariances, a bound that
// does not settle the far-list test, a mean outside the candidate margins -- makes the WAVE take the usual body for the pair instead
// (returns false, wave-uniform; nothing has been written by then), which then does exactly what it always did.
// bnd: the bounds the landmarks' lists were pruned with (Kb, Ib; Ib = 0: nothing to hold).
__device__ __forceinline__ bool pub_lean_pair(PubSlots (&q)[2], double (&pse_out)[2], const PubGateIn (&in)[2],
                                              const Landmark<double>* const (&lmp)[2], const float2 (&bnd)[2], const double* ex,
                                              unsigned char* any, unsigned anydump, double sx, double sy, double sh) {
  constexpr double ln2 = 0.69314718055994530942;
  bool unsure = false, positive[2];
  unsigned t[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const Landmark<double>& lm = *lmp[j];
    const double pse = pk_atan2(in[j].my - sy, in[j].mx - sx);
    pse_out[j] = pse;
    const double eb = pse - sh;  // :408
    const double deb = eb - (double)__uint_as_float(in[j].ref.x);
    const bool inside = (fabs(deb) <= kCandBearing || fabs(deb - Consts<double>::two_pi) <= kCandBearing ||
                         fabs(deb + Consts<double>::two_pi) <= kCandBearing) &&
                        fabs(in[j].mr - (double)__uint_as_float(in[j].ref.y)) <= kCandColour &&
                        fabs(in[j].mg - (double)__uint_as_float(in[j].ref.z)) <= kCandColour &&
                        fabs(in[j].mb - (double)__uint_as_float(in[j].ref.w)) <= kCandColour;  // (pub_gatesN's test; NaN: outside)
    t[j] = in[j].has ? (in[j].cw[0].x & 0xFFFFu) : 0xFFFFu;
    const bool valid = t[j] != 0xFFFFu;
    const double* rec = ex + 6 * (valid ? t[j] : 0u);
    const double2 z01 = *reinterpret_cast<const double2*>(rec);
    const double2 z23 = *reinterpret_cast<const double2*>(rec + 2);
    const double2 dir = *reinterpret_cast<const double2*>(rec + 4);
    const double cd = color_distance2(in[j].mr, in[j].mg, in[j].mb, z01.y, z23.x, z23.y);
    const bool pass = valid && !(fabs(z01.x - eb) > 0.5) && !(fabs(cd) > 300.0);  // :433, :441
    // pub_keysN's prologue, without the logarithm
    const double det2 = lm.pxx * lm.pyy - lm.pxy * lm.pxy;
    double det3;
    const Sym3<double> adj3 = sym3_adjugate(Sym3<double>{lm.crr, lm.crg, lm.crb, lm.cgg, lm.cgb, lm.cbb}, det3);
    const bool sane = det2 > 1e-20 && det2 < 1e60 && det3 > 1e-20 && det3 < 1e60;  // NaN: false
    int e2i, e3i;
    (void)frexp(det2, &e2i);
    (void)frexp(det3, &e3i);
    const double a2base = 2.0 * Consts<double>::log_two_pi + (double)e2i * ln2;
    const double a3base = 3.0 * Consts<double>::log_two_pi + (double)e3i * ln2;
    const double khi = a2base + a3base, klo = khi - 2.0 * ln2;  // klo <= 5 log 2 pi + log(det2 det3) <= khi
    bool pd3;
    const double itr3 = pub_far_slope(lm, sane, det2, det3, adj3.f, pd3);
    // the landmark's own far bound against the scan's (pub_keysN<CHK>): certain only with room for pub_log's error (1e-12)
    const bool holds = itr3 >= (double)bnd[j].y && klo >= (double)bnd[j].x + 1e-9;
    // the verdict (pub_keysN's round): certain on either side of the strip 1489 ... 1491.5, which the usual body evaluates exactly
    const bool angle_ok = !(fabs(pse - z01.x) > Consts<double>::half_pi);  // :473-475
    double nx, ny;
    closest_point(lm.mx, lm.my, sx, sy, dir.x, dir.y, nx, ny);
    const double ex_ = nx - lm.mx, ey = ny - lm.my;
    const double d1 = z01.y - lm.mr, d2c = z23.x - lm.mg, d3c = z23.y - lm.mb;
    const double num2 = lm.pyy * ex_ * ex_ - 2.0 * lm.pxy * ex_ * ey + lm.pxx * ey * ey;
    const double num3 = sym3_quad(adj3, d1, d2c, d3c);
    const double maha2 = num2 * pub_recip(det2), maha3 = num3 * pub_recip(det3);
    const bool nonneg = fmin(num2, num3) >= 0.0;  // NaN: false
    const double amax = fmax(a2base + maha2, a3base + maha3);
    const bool sure_pos = angle_ok && nonneg && fmax(khi + (maha2 + maha3), amax) < 1489.0;
    const bool sure_zero = !angle_ok || klo + (maha2 + maha3) > 1491.5;
    positive[j] = pass && sure_pos;
    unsure |= in[j].has && (!inside || !holds || (pass && (!sane || (angle_ok && !nonneg) || (!sure_pos && !sure_zero))));
    q[j] = kPubNoSlots;
    q[j].s[0] = pass ? (t[j] | 0xFFFF0000u) : 0xFFFFFFFFu;
    q[j].st = positive[j] ? 5u : 0u;  // probability > 0, and taken: nobody else lists the blob
  }
  if (__ballot(unsure) != 0ull) return false;  // wave-uniform
#pragma unroll
  for (int j = 0; j < 2; ++j) any[positive[j] ? t[j] : anydump] = 1;
  return true;
}

#ifdef PK_STAMPS
__device__ unsigned long long pk_pstamp_acc[16];  // (diagnostic build: per-phase cycle sums and counters, see below)
#endif
// What pub_keysN needs to test that the scan's pruned lists hold for its landmarks (CHK), as FUNCTIONS evaluated where the
// values are used -- held in registers from the call on they cost k_step_pub<2, 512>, which sits at 256 VGPRs, 70-100 spills:
// bnd(j): the bound landmark j's list was pruned with (Kb, Ib; Ib = 0: an empty far list, nothing to hold); has(j): the landmark
// exists; far_row(): the pair's far records [hdr | list x W4] x N, or null; sh: the heading.
struct PubNoChk {
  __device__ __forceinline__ float2 bnd(int) const { return make_float2(-3.0e38f, 0.f); }
  __device__ __forceinline__ bool has(int) const { return false; }
  __device__ __forceinline__ const uint4* far_row() const { return nullptr; }
  double sh = 0.0;
};
// Verdicts of the two landmarks of a pair on their gate-passing blobs: published for the blobs other landmarks list too,
// any[t] = 1 where the probability is > 0 (the blob will be matched by somebody: no 0.1 factor, :94-95).  any[anydump]: a
// byte nobody reads.  One slot of each landmark per round, side by side (two independent chains).
// PRE: kbase and 1 / rowmax come from the caller (pub_far_bound, k_step_pub_big: its gates needed them already)
// (Measured and dropped, round 4: look-alikes certainly beyond the underflow edge taken out of slots 1.. before the rounds, +11 % --
// profiles/r04/ab_pub_prune_far_slots.log; any[] as COUNTERS of the landmarks that want a blob, so that a blob with one taker
// needs no settling, +0.6 % -- ab_counted_settling.log.)
// CHK: the lists have had their far look-alikes taken off (k_candidates): the landmarks' own bounds are held against the scan's
// (pub_far_recheck), W4F uint4 words per far list
// PRIM: a round in which every lane's blob is its landmark's primary one reads the records from the primary-blob table (prim)
template <int N, int SL = kPubSlots, bool PRE = false, bool CHK = false, int W4F = 1, class Chk = PubNoChk, bool PRIM = false>
__device__ __forceinline__ void pub_keysN(PubSlotsT<SL> (&q)[N], const Landmark<double>* const (&lmp)[N],
                                          const double (&pse)[N], const double* ex, double* pub, unsigned dump, unsigned char* any,
                                          unsigned anydump, int* flag, double sx, double sy, const double* pre_kbase = nullptr,
                                          const double* pre_itr3 = nullptr, const Chk& chk = Chk(), const PubPrim* prim = nullptr) {
  bool nobody;  // wave-uniform: nobody's landmark passes a blob
  {
    unsigned sall = q[0].s[0];
#pragma unroll
    for (int j = 1; j < N; ++j) sall &= q[j].s[0];
    nobody = __ballot((sall & 0xFFFFu) != 0xFFFFu) == 0ull;
    if (nobody) {
      // (... of its pruned list: a landmark with a far list still has to hold its own bound against the scan's -- the wave goes
      // through the prologue for that and leaves behind the test; rare: a wave none of whose 128 landmarks sees a blob it could match)
      bool need = false;
      if constexpr (CHK) {
#pragma unroll
        for (int j = 0; j < N; ++j) need |= chk.has(j) && chk.bnd(j).y > 0.f;
      }
      if (!CHK || __ballot(need) == 0ull) return;
    }
  }
  constexpr double ln2 = 0.69314718055994530942;
  double det2[N], det3[N], r2[N], r3[N], a2base[N], a3base[N], kbase[N], itr3[N];
  Sym3<double> adj3[N];
  bool sane[N], pd3[N];
  bool weird = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const Landmark<double>& lm = *lmp[j];
    det2[j] = lm.pxx * lm.pyy - lm.pxy * lm.pxy;
    adj3[j] = sym3_adjugate(Sym3<double>{lm.crr, lm.crg, lm.crb, lm.cgg, lm.cgb, lm.cbb}, det3[j]);
    // (determinants within 1e-20 ... 1e60: then log det >= -46, and a pair with a subnormal factor -- a2 or a3 beyond 1400
    // -- has a key beyond 1350: the settling tells fragile winners by their key alone)
    sane[j] = det2[j] > 1e-20 && det2[j] < 1e60 && det3[j] > 1e-20 && det3[j] < 1e60;  // NaN: false
    r2[j] = pub_recip(det2[j]);
    r3[j] = pub_recip(det3[j]);
    // log det = (e + log2 m) ln 2 with m in [0.5, 1): bounded above by e ln 2, below by (e - 1) ln 2 -- all the underflow
    // tests need of the two logs; the key itself takes ONE log, of the product
    int e2i, e3i;
    (void)frexp(det2[j], &e2i);
    (void)frexp(det3[j], &e3i);
    a2base[j] = 2.0 * Consts<double>::log_two_pi + (double)e2i * ln2;  // >= 2 log 2pi + log det2
    a3base[j] = 3.0 * Consts<double>::log_two_pi + (double)e3i * ln2;
    if constexpr (PRE)
      kbase[j] = pre_kbase[j];
    else
      kbase[j] = 5.0 * Consts<double>::log_two_pi + pub_log(det2[j] * det3[j]);
    // A colour block that is certainly positive definite (Sylvester) has d' C^-1 d >= |d|^2 / lmax(C), and lmax(C) is at
    // most the largest absolute row sum (Gershgorin): with the position term >= 0 that bounds the key from below by
    // kbase + |d|^2 / rowmax, and a blob whose bound lies beyond the underflow edge has probability 0 whatever the rest
    // says.  Once a landmark has been seen a few times its colour block is tight and every look-alike's blob ends here:
    // when that holds for all lanes of the wave the round's arithmetic is skipped
    // (both blocks CERTAINLY positive definite: pub_far_slope, pk_pub_math.hpp -- the one statement of it; the caller's value
    // came from there too, through pub_far_bound)
    if constexpr (PRE) {
      itr3[j] = pre_itr3[j];
      pd3[j] = itr3[j] > 0.0;
    } else {
      itr3[j] = pub_far_slope(lm, sane[j], det2[j], det3[j], adj3[j].f, pd3[j]);
    }
  }
  if constexpr (CHK) {
    bool viol[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float2 b = chk.bnd(j);
      viol[j] = chk.has(j) && !(itr3[j] >= (double)b.y && kbase[j] >= (double)b.x);
    }
    pub_far_recheck<N, W4F>(viol, lmp, pse, kbase, itr3, [&]() { return chk.far_row(); }, ex, chk.sh, flag);
    if (nobody) return;
  }
  int done = 0;
#pragma unroll 1
  for (; done < SL; ++done) {
    unsigned sall = q[0].s[0];
#pragma unroll
    for (int j = 1; j < N; ++j) sall &= q[j].s[0];
    if (__ballot((sall & 0xFFFFu) != 0xFFFFu) == 0ull) break;  // wave-uniform: every landmark is through
    unsigned t[N], e[N];
    bool valid[N], far[N], positive[N];
    double2 z01[N], z23[N];
    double d1[N], d2c[N], d3c[N];
    const double* rec[N];
    // PRIM: the blob's three 16-byte words stand at rb0 + roff, + rks, + 2 rks -- in the scan's records (48-byte records, blob by blob:
    // a gather) or, in a round in which EVERY lane's blob is its landmark's primary one (wave-uniform: the first round, nearly always),
    // in the primary-blob table (planes in landmark order: neighbouring lanes, neighbouring addresses).  One code path, a uniform base
    // and a 32-bit offset per landmark: no register more than the gather took.
    unsigned roff[N];
    const char* rb0 = nullptr;
    size_t rks = 0;
    if constexpr (PRIM) {
      bool offp = false;
#pragma unroll
      for (int j = 0; j < N; ++j) offp |= (q[j].s[0] & 0xFFFFu) != 0xFFFFu && (q[j].s[0] & 0xFFFFu) != prim->t0(j);
      const bool onp = __ballot(offp) == 0ull;
      rb0 = onp ? reinterpret_cast<const char*>(prim->tab + prim->Lpp) : reinterpret_cast<const char*>(ex);
      rks = onp ? prim->Lpp * 16 : (size_t)16;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const unsigned tj = q[j].s[0] & 0xFFFFu;
        roff[j] = onp ? (unsigned)(prim->lc + j) * 16u : (tj != 0xFFFFu ? tj : 0u) * 48u;
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const Landmark<double>& lm = *lmp[j];
      t[j] = q[j].s[0] & 0xFFFFu;
      e[j] = q[j].s[0] >> 16;
      valid[j] = t[j] != 0xFFFFu;
      if constexpr (PRIM) {
        z01[j] = *reinterpret_cast<const double2*>(rb0 + roff[j]);
        z23[j] = *reinterpret_cast<const double2*>(rb0 + rks + roff[j]);
      } else {
        rec[j] = ex + 6 * (valid[j] ? t[j] : 0u);
        z01[j] = *reinterpret_cast<const double2*>(rec[j]);
        z23[j] = *reinterpret_cast<const double2*>(rec[j] + 2);
      }
      d1[j] = z01[j].y - lm.mr;
      d2c[j] = z23[j].x - lm.mg;
      d3c[j] = z23[j].y - lm.mb;
      far[j] = pd3[j] && kbase[j] + (d1[j] * d1[j] + d2c[j] * d2c[j] + d3c[j] * d3c[j]) * itr3[j] > 1492.0;  // key > 1492: probability 0
      positive[j] = false;
    }
    bool heavy = false;
#pragma unroll
    for (int j = 0; j < N; ++j) heavy |= valid[j] && !far[j];
#if defined(PK_STAMPS) && defined(PK_DIAG_ROUNDS)
    if constexpr (PRIM) {  // (diagnostic: how full are the verdict rounds of the two-pass kernel -- DESIGN.md section 10.2)
      unsigned long long act = 0ull;
#pragma unroll
      for (int j = 0; j < N; ++j) act += (unsigned long long)__popcll(__ballot(valid[j] && !far[j]));
      if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u) {
        if (done == 0) atomicAdd(&pk_pstamp_acc[12], 1ull);
        if (act != 0ull) atomicAdd(&pk_pstamp_acc[13], 1ull);
        if (act != 0ull && done > 0) atomicAdd(&pk_pstamp_acc[14], 1ull);
        if (done > 0) atomicAdd(&pk_pstamp_acc[15], act);
      }
    }
#endif
    if (__ballot(heavy) != 0ull) {  // wave-uniform
      double key[N], num2[N], num3[N];
      bool edge[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const Landmark<double>& lm = *lmp[j];
        double2 dir;
        if constexpr (PRIM)
          dir = *reinterpret_cast<const double2*>(rb0 + 2 * rks + roff[j]);
        else
          dir = *reinterpret_cast<const double2*>(rec[j] + 4);
        // prob_position_match :457-494, prob_color_match :524-544
        const bool angle_ok = !(fabs(pse[j] - z01[j].x) > Consts<double>::half_pi);  // :473-475
        double nx, ny;
        closest_point(lm.mx, lm.my, sx, sy, dir.x, dir.y, nx, ny);
        const double ex_ = nx - lm.mx, ey = ny - lm.my;
        num2[j] = lm.pyy * ex_ * ex_ - 2.0 * lm.pxy * ex_ * ey + lm.pxx * ey * ey;  // maha2 = num2 / det2
        num3[j] = sym3_quad(adj3[j], d1[j], d2c[j], d3c[j]);                         // maha3 = num3 / det3
        const double maha2 = num2[j] * r2[j], maha3 = num3[j] * r3[j];
        key[j] = kbase[j] + (maha2 + maha3);
        const double a2hi = a2base[j] + maha2, a3hi = a3base[j] + maha3;
        // pr = fl(fl(bp cp) / 250000), bp = 500 exp(-a2 / 2), cp = 500 exp(-a3 / 2): bp rounds to 0 from a2 > 1490.27 on
        // (exp(-745.13) = 2^-1075, half the smallest subnormal), the quotient from a2 + a3 > 1490.27 on.  Outside the
        // margins below the answer is certain; inside (a strip 2.5-3.2 wide) the probability is evaluated as the reference does
        const bool nonneg = fmin(num2[j], num3[j]) >= 0.0;  // indefinite covariances, NaN: false
        weird |= valid[j] && (!sane[j] || (angle_ok && !nonneg));
        const double amax = fmax(a2hi, a3hi);
        const bool sure_pos = angle_ok && nonneg && fmax(key[j], amax) < 1489.0;
        const bool sure_zero = !angle_ok || fmax(key[j], amax - ln2) > 1491.5;
        positive[j] = valid[j] && sure_pos;
        edge[j] = valid[j] && !sure_pos && !sure_zero;
      }
      bool anyedge = false;
#pragma unroll
      for (int j = 0; j < N; ++j) anyedge |= edge[j];
      if (__ballot(anyedge) != 0ull) {  // wave-uniform, rare
#pragma unroll
        for (int j = 0; j < N; ++j)
          if (edge[j]) {
            double d2 = det2[j], d3 = det3[j];
            asm volatile("" : "+v"(d2), "+v"(d3));  // opaque: keeps the logs and exps of this rare branch out of the common path
            positive[j] = pr_from_parts(d2, d3, num2[j], num3[j]) > 0.0;
          }
      }
#pragma unroll
      for (int j = 0; j < N; ++j) pub[(e[j] == 0xFFFFu) ? dump : e[j]] = positive[j] ? key[j] : pub_inf();  // (an empty slot's entry field is 0xFFFF)
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        weird |= valid[j] && !sane[j];
        pub[(e[j] == 0xFFFFu) ? dump : e[j]] = pub_inf();
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      any[positive[j] ? t[j] : anydump] = 1;
      q[j].st |= positive[j] ? 1u : 0u;
      pub_rotate(q[j]);
    }
  }
  for (; done < SL; ++done) {  // wave-uniform trip count: back to the original order
#pragma unroll
    for (int j = 0; j < N; ++j) pub_rotate(q[j]);
  }
  if (weird) *flag = 1;
}

// Landmarks that passed MORE blobs than they have slots (pub_gatesN<OVF>; a few landmarks of some particles, at some poses).
// The slots hold the last kPubSlots blobs that passed and pub_keysN has given those their verdicts; the blobs the slots no
// longer hold take the places of slots whose blob turned out to have probability 0 (a look-alike's, beyond the underflow edge
// once the landmark's colour block has tightened: nearly always all but one), and the caller runs pub_keysN ONCE MORE on the
// refilled slots -- the same code in a loop, so the usual case pays nothing for this and no register is held for it; a slot
// that keeps its blob publishes the same values again.  Blobs left over when the free slots run out: the particle goes to the
// fall-back kernels, as it did for any fifth blob before round 4.  Returns false when no lane of the wave has such a landmark
// (wave-uniform).
// W4: uint4 words per list (1: eight candidates, records [ref | list] and one entry word; 2: sixteen, [ref | list | list] and two)
template <int N, int W4 = 1>
__device__ __forceinline__ bool pub_refill_slots(PubSlots (&q)[N], const uint4* cand_row, const uint4* erec_row, int* flag) {
  bool anyovf = false;
#pragma unroll
  for (int j = 0; j < N; ++j) anyovf |= __popc(q[j].st >> 16) > kPubSlots;
  if (__ballot(anyovf) == 0ull) return false;  // wave-uniform: the usual case
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const unsigned pmask = q[j].st >> 16;
    const bool ovf = __popc(pmask) > kPubSlots;
    if (__ballot(ovf) == 0ull) continue;  // wave-uniform
    // this landmark's list words once more (L2), one word -- two candidates -- at a time
    const unsigned* cwp = reinterpret_cast<const unsigned*>(cand_row + (1 + W4) * j + 1);
    const unsigned* ewp = reinterpret_cast<const unsigned*>(erec_row + W4 * j);
    const unsigned id0 = q[j].s[0] & 0xFFFFu, id1 = q[j].s[1] & 0xFFFFu, id2 = q[j].s[2] & 0xFFFFu, id3 = q[j].s[3] & 0xFFFFu;
    unsigned open = ~q[j].st & 0x1111u;  // slots whose blob has probability 0: its verdict is out, the place is free
#pragma unroll 1
    for (int w = 0; w < W4 * kCandSlots / 2; ++w) {
      const unsigned cw = cwp[w], ew = ewp[w];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const unsigned t = (cw >> (16 * half)) & 0xFFFFu, e = (ew >> (16 * half)) & 0xFFFFu;
        const bool extra = ovf && ((pmask >> (2 * w + half)) & 1u) != 0u && t != id0 && t != id1 && t != id2 && t != id3;
        if (extra && open == 0u) *flag = 1;
        const unsigned word = t | (e << 16);
        bool placed = !extra;
#pragma unroll
        for (int sidx = 0; sidx < kPubSlots; ++sidx) {
          const bool here = !placed && ((open >> (4 * sidx)) & 1u) != 0u;
          q[j].s[sidx] = here ? word : q[j].s[sidx];
          open &= here ? ~(1u << (4 * sidx)) : ~0u;
          placed |= here;
        }
      }
    }
    q[j].st &= 0xFFFFu;  // the mask has done its work: a second refill finds nothing
  }
  return true;
}

// Settling, BLOB-parallel: one lane per blob that several landmarks list (a few per lane, their entries one contiguous
// run of the table, read in one batch).  The smallest key takes the blob, the lowest landmark -- the lowest rank -- on
// equal keys (:377); its entry is overwritten with the marker -inf, which is what the landmark's lane looks for afterwards.
// Too close to call on keys (two contenders within 1e-7 that are not identical), or a winner whose probability is
// subnormal (key beyond 1350: keys order such probabilities only roughly) next to another contender: the particle is
// flagged and the general kernels compare probabilities.  (A first version let every landmark's lane read its rivals'
// entries one after the other: 40 % of the kernel's time went into those dependent LDS round trips.)
__device__ __forceinline__ double pub_marker() { return __longlong_as_double((long long)0xFFF0000000000000ull); }
template <int THREADS, int SLOTS = kCandSlots>
__device__ __forceinline__ void pub_settle_blobs(int tid, const unsigned* glist, unsigned G, double* pub, unsigned dump, int* flag,
                                                 const unsigned* rb) {
  constexpr bool kRankMajor = SLOTS > kCandSlots;
  // (TWO blobs per lane and turn, side by side: +1.1 %, profiles/r04/ab_settle_two_blobs_per_turn.log)
  constexpr int TWO = 1;
  // (most contested blobs are listed by two or three landmarks: the first four entries in one batch, the rest -- wave-uniform --
  // only where some lane's blob has more; round 4: the settling read and compared all SLOTS entries of every blob)
  constexpr int kHead = SLOTS < 4 ? SLOTS : 4;
  constexpr int kMid = SLOTS > 8 ? 8 : SLOTS;
  bool doubt = false;
#pragma unroll 1
  for (unsigned g0 = (unsigned)tid; __ballot(g0 < G) != 0ull; g0 += TWO * THREADS) {  // wave-uniform
    unsigned g[TWO], n[TWO], offs[TWO], wr[TWO];
    double v[TWO][SLOTS], best[TWO];
    // entry of (blob, rank r): rank-major rb[r] + g (the lanes of a wave read consecutive words; every contested blob has ranks 0
    // and 1: their bases are 0 and G), blob-major offs + r
    auto entry = [&](int h, int r) -> unsigned {
      return kRankMajor ? (r == 0 ? g[h] : r == 1 ? G + g[h] : rb[r] + g[h]) : offs[h] + (unsigned)r;
    };
#pragma unroll
    for (int h = 0; h < TWO; ++h) {
      g[h] = g0 + (unsigned)h * THREADS;
      const bool on = g[h] < G;
      const unsigned gi = glist[on ? g[h] : 0u];
      offs[h] = gi & 0xFFFFu;
      n[h] = on ? (gi >> 16) : 0u;
    }
#pragma unroll
    for (int h = 0; h < TWO; ++h)
#pragma unroll
      for (int r = 0; r < kHead; ++r) v[h][r] = pub[(unsigned)r < n[h] ? entry(h, r) : dump];
    bool anymore = false, anymost = false;
#pragma unroll
    for (int h = 0; h < TWO; ++h) {
      best[h] = pub_inf();
      wr[h] = 0u;
#pragma unroll
      for (int r = 0; r < kHead; ++r) {
        v[h][r] = (unsigned)r < n[h] ? v[h][r] : pub_inf();
        const bool better = v[h][r] < best[h];  // strict: on equal keys the earlier rank stays (:377)
        wr[h] = better ? (unsigned)r : wr[h];
        best[h] = better ? v[h][r] : best[h];
      }
      anymore |= n[h] > (unsigned)kHead;
      anymost |= n[h] > (unsigned)kMid;
    }
    const bool more = SLOTS > kHead && __ballot(anymore) != 0ull;  // wave-uniform
    const bool most = SLOTS > kMid && __ballot(anymost) != 0ull;
    if (more) {
#pragma unroll
      for (int h = 0; h < TWO; ++h)
#pragma unroll
        for (int r = kHead; r < kMid; ++r) v[h][r] = pub[(unsigned)r < n[h] ? entry(h, r) : dump];
#pragma unroll
      for (int h = 0; h < TWO; ++h)
#pragma unroll
        for (int r = kHead; r < kMid; ++r) {
          v[h][r] = (unsigned)r < n[h] ? v[h][r] : pub_inf();
          const bool better = v[h][r] < best[h];
          wr[h] = better ? (unsigned)r : wr[h];
          best[h] = better ? v[h][r] : best[h];
        }
    }
    if (most) {
#pragma unroll
      for (int h = 0; h < TWO; ++h)
#pragma unroll
        for (int r = kMid; r < SLOTS; ++r) v[h][r] = pub[(unsigned)r < n[h] ? entry(h, r) : dump];
#pragma unroll
      for (int h = 0; h < TWO; ++h)
#pragma unroll
        for (int r = kMid; r < SLOTS; ++r) {
          v[h][r] = (unsigned)r < n[h] ? v[h][r] : pub_inf();
          const bool better = v[h][r] < best[h];
          wr[h] = better ? (unsigned)r : wr[h];
          best[h] = better ? v[h][r] : best[h];
        }
    }
#pragma unroll
    for (int h = 0; h < TWO; ++h) {
      int contenders = 0;
      bool close = false;
#pragma unroll
      for (int r = 0; r < kHead; ++r) {
        contenders += v[h][r] < pub_inf() ? 1 : 0;
        close |= v[h][r] != best[h] && v[h][r] - best[h] < 1e-7;  // within 1e-7 of the winner without being identical to it
      }
      if (more) {
#pragma unroll
        for (int r = kHead; r < kMid; ++r) {
          contenders += v[h][r] < pub_inf() ? 1 : 0;
          close |= v[h][r] != best[h] && v[h][r] - best[h] < 1e-7;
        }
      }
      if (most) {
#pragma unroll
        for (int r = kMid; r < SLOTS; ++r) {
          contenders += v[h][r] < pub_inf() ? 1 : 0;
          close |= v[h][r] != best[h] && v[h][r] - best[h] < 1e-7;
        }
      }
      doubt |= close || (contenders >= 2 && best[h] > 1350.0);
    }
#pragma unroll
    for (int h = 0; h < TWO; ++h) {  // (the two blobs' entries are disjoint: the markers go out behind every read of the turn)
      unsigned we = kRankMajor ? g[h] : offs[h] + wr[h];
      if constexpr (kRankMajor) we += wr[h] == 0u ? 0u : wr[h] == 1u ? G : rb[wr[h]];
      pub[best[h] < pub_inf() ? we : dump] = best[h] < pub_inf() ? pub_marker() : pub_inf();
    }
  }
  if (doubt) *flag = 1;
}

// Which of its blobs this landmark takes: those it passes with probability > 0 and either nobody else lists, or whose
// entry carries the winner's marker.
__device__ __forceinline__ void pub_take(PubSlots& q, const double* pub, unsigned dump) {
  const unsigned sw[kPubSlots] = {q.s[0], q.s[1], q.s[2], q.s[3]};
  double m[kPubSlots];
#pragma unroll
  for (int s = 0; s < kPubSlots; ++s) {
    const unsigned e = sw[s] >> 16;
    m[s] = pub[e == 0xFFFFu ? dump : e];
  }
#pragma unroll
  for (int s = 0; s < kPubSlots; ++s) {
    const unsigned e = sw[s] >> 16;
    const bool pos = ((q.st >> (4 * s)) & 1u) != 0u;
    if (pos && (e == 0xFFFFu || m[s] == pub_marker())) q.st |= 4u << (4 * s);
  }
}

// One logarithm per lane and particle for the importance factors' norms (:844-849; ekf_update's fro_prod; round 6): the product of the
// squared Frobenius norms of the lane's updates is folded into the log-weight -- -1/4 log(prod) -- behind the lane's last update.
// ekf_update looks at the product behind every single factor and keeps it a positive normal number whatever Qt and the covariances
// are (a look once per landmark pair, at a window of [1e-150, 1e150], let eight factors of 3e40, Qt = 1e20 I, through to infinity:
// log-weights of -inf from these kernels, -24 an update from the others), so there is nothing to look at in between.
// The logarithm is 45 of an update's 300 float64 instructions: k_step_pub
// 7.91 -> 7.71 ms at 100 000 x 2 000 (-2.4 %), k_step_pub_big 5.75 -> 5.71 ms at 20 000 x 5 000 (profiles/r06/ab_one_log_per_lane_*.log;
// PK_DIAG_LOG_PER_UPDATE is the regression build).  The log-weights differ from a logarithm per update in the last bits only.
#ifndef PK_DIAG_LOG_PER_UPDATE
#define PK_PROD_PTR(p_) (&(p_))
#else
#define PK_PROD_PTR(p_) ((double*)nullptr)
#endif
__device__ __forceinline__ void pub_fold_norms(double& acc, double& prod) {
#ifndef PK_DIAG_LOG_PER_UPDATE
  acc -= 0.25 * log_few_ulp(prod);  // (a NaN stays what the sum of logarithms was: NaN)
  prod = 1.0;
#else
  (void)acc;
  (void)prod;
#endif
}
// The blobs taken, applied in scan order (:88): regs_apply with the take bits.
// TAB (the colour table stands for the slots' colour rows): a landmark's ONLY update of the scan leaves its colour block alone -- the
// kernel does not store it; a landmark that takes several blobs carries the block from update to update in registers as ever
template <bool TAB = false>
__device__ __forceinline__ double pub_apply(const PubSlots& q, const double* ex, const unsigned short* order, const Noise<double>& qt,
                                            Landmark<double>& lm, bool imm, double sx, double sy, double pse, double* prod = nullptr) {
  double acc = 0.0;
  const unsigned tk = q.st & 0x4444u;
  if (__ballot(tk != 0u) == 0ull) return acc;  // wave-uniform
  if (__ballot((tk & (tk - 1u)) != 0u) == 0ull) {
    // wave-uniform, the usual case: no landmark takes more than one blob -- no scan-order sort, no loop
    if (tk != 0u) {
      const unsigned w = (tk & 0x0004u) ? q.s[0] : (tk & 0x0040u) ? q.s[1] : (tk & 0x0400u) ? q.s[2] : q.s[3];
      const double* rec = ex + 6 * (w & 0xFFFFu);
      const double2 z01 = *reinterpret_cast<const double2*>(rec);
      const double2 z23 = *reinterpret_cast<const double2*>(rec + 2);
      BlobT<double> z{z01.x, z01.y, z23.x, z23.y};
      acc = ekf_update<double, !TAB>(lm, sx, sy, z, qt, imm, (EkfAux<double>*)nullptr, &pse, prod);
    }
    return acc;
  }
  const unsigned sw[kPubSlots] = {q.s[0], q.s[1], q.s[2], q.s[3]};
  unsigned key[kPubSlots];
#pragma unroll
  for (int s = 0; s < kPubSlots; ++s) {
    const bool take = ((q.st >> (4 * s)) & 4u) != 0u;
    const unsigned t = sw[s] & 0xFFFFu;
    const unsigned o = order[take ? t : 0u];
    key[s] = take ? ((o << 16) | t) : 0xFFFFFFFFu;
  }
  auto cswap = [&](unsigned& u, unsigned& v) {
    const unsigned lo = min(u, v), hi = max(u, v);
    u = lo;
    v = hi;
  };
  cswap(key[0], key[1]);
  cswap(key[2], key[3]);
  cswap(key[0], key[2]);
  cswap(key[1], key[3]);
  cswap(key[1], key[2]);
  bool fresh = true;
#pragma unroll 1
  for (int it = 0; it < kPubSlots; ++it) {
    const unsigned kk = key[0];
    if (__ballot(kk != 0xFFFFFFFFu) == 0ull) break;  // wave-uniform
    key[0] = key[1];
    key[1] = key[2];
    key[2] = key[3];
    key[3] = 0xFFFFFFFFu;
    if (kk != 0xFFFFFFFFu) {
      const double* rec = ex + 6 * (kk & 0xFFFFu);
      const double2 z01 = *reinterpret_cast<const double2*>(rec);
      const double2 z23 = *reinterpret_cast<const double2*>(rec + 2);
      BlobT<double> z{z01.x, z01.y, z23.x, z23.y};
      acc += ekf_update(lm, sx, sy, z, qt, imm, (EkfAux<double>*)nullptr, fresh ? &pse : (const double*)nullptr, prod);
      fresh = imm;
    }
  }
  return acc;
}

// The same with ONE copy of the update code, in a loop that nearly always turns once (the 256-lane instance: 145 VGPRs
// instead of 181; on the large instance 0.7 % slower than the two-path form above).
// PRIM: a turn in which every lane applies its landmark's primary blob (t0; nearly always) reads that blob's exact record from the
// primary-blob table -- ptab its plane 1 (uniform), pstride the planes' stride in bytes, pidx the landmark -- instead of gathering
template <bool PRIM = false>
__device__ __forceinline__ double pub_apply_loop(const PubSlots& q, const double* ex, const unsigned short* order, const Noise<double>& qt,
                                            Landmark<double>& lm, bool imm, double sx, double sy, double pse,
                                            const char* ptab = nullptr, size_t pstride = 0, int pidx = 0, unsigned t0 = 0xFFFFu,
                                            double* prod = nullptr) {
  double acc = 0.0;
  unsigned tk = q.st & 0x4444u;
  bool fresh = true;
#pragma unroll 1
  for (int it = 0; it < kPubSlots; ++it) {
    if (__ballot(tk != 0u) == 0ull) break;  // wave-uniform
    unsigned w, bit;
    if (__ballot((tk & (tk - 1u)) != 0u) == 0ull) {  // wave-uniform, the usual case: at most one blob left per landmark
      w = (tk & 0x0004u) ? q.s[0] : (tk & 0x0040u) ? q.s[1] : (tk & 0x0400u) ? q.s[2] : q.s[3];
      bit = tk;
    } else {  // the one that comes first in the scan
      const unsigned sw[kPubSlots] = {q.s[0], q.s[1], q.s[2], q.s[3]};
      unsigned best = 0xFFFFFFFFu;
      w = 0u;
      bit = 0u;
#pragma unroll
      for (int s = 0; s < kPubSlots; ++s) {
        const bool on = ((tk >> (4 * s)) & 4u) != 0u;
        const unsigned o = order[on ? (sw[s] & 0xFFFFu) : 0u];
        const bool first = on && o < best;
        best = first ? o : best;
        w = first ? sw[s] : w;
        bit = first ? (4u << (4 * s)) : bit;
      }
    }
    const char* rb0 = reinterpret_cast<const char*>(ex);
    size_t rks = 16;
    bool onp = false;  // wave-uniform
    if constexpr (PRIM) {
      onp = __ballot(tk != 0u && (w & 0xFFFFu) != t0) == 0ull;
      rb0 = onp ? ptab : rb0;
      rks = onp ? pstride : rks;
    }
    if (tk != 0u) {
      const unsigned roff = (PRIM && onp) ? (unsigned)pidx * 16u : (w & 0xFFFFu) * 48u;
      const double2 z01 = *reinterpret_cast<const double2*>(rb0 + roff);
      const double2 z23 = *reinterpret_cast<const double2*>(rb0 + rks + roff);
      BlobT<double> z{z01.x, z01.y, z23.x, z23.y};
      acc += ekf_update(lm, sx, sy, z, qt, imm, (EkfAux<double>*)nullptr, fresh ? &pse : (const double*)nullptr, prod);
      fresh = imm;
    }
    tk &= ~bit;
  }
  return acc;
}

// Diagnostic build only (-DPK_STAMPS): per-phase cycle sums of k_step_pub (slots 48.. of pk_debug_stamps).
#ifdef PK_STAMPS
__device__ unsigned long long pk_pstamp_wave[8][12];  // the same sums per wave of the workgroup (which waves wait at the barriers?)
// (summed in scalar registers, one atomic per wave and slot at the very end: an atomic per stamp put 2 048 waves in a
// queue for sixteen addresses and, the vector memory counter being one in-order counter, every row behind them)
#define PK_PSTAMP(slot, a, b) pst[slot] += (b) - (a);
void debug_read_pub_wave_stamps(unsigned long long* out, bool reset) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(pk_pstamp_wave), sizeof(unsigned long long) * 96);
  if (reset) {
    unsigned long long z[96] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(pk_pstamp_wave), z, sizeof(z));
  }
}
void debug_read_pub_stamps(unsigned long long* out, bool reset) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(pk_pstamp_acc), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(pk_pstamp_acc), z, sizeof(z));
  }
}
#else
#define PK_PSTAMP(slot, a, b)
#endif

// ------------------------------------------------------------------ the kernel
// The kernel's arguments are read from the kernarg segment where they are needed, phase by phase, instead of sitting in
// ~80 SGPRs for the whole particle loop (the register allocator spilled 108 of them into VGPR lanes): an empty asm makes
// the pointer opaque, so that nothing loaded through it before is kept alive across it.
typedef const __attribute__((address_space(4))) PubArgs* PubArgsPtr;
__device__ __forceinline__ PubArgsPtr pub_args_now(PubArgsPtr rp) {
  asm volatile("" : "+s"(rp));
  return rp;
}
__device__ __forceinline__ SlotSource pub_slot_source(PubArgsPtr R) {
  return SlotSource{R->ss.map, R->ss.slot_bytes, R->ss.alt, R->ss.alt_stride, R->ss.alt_off};
}
__device__ __forceinline__ Noise<double> pub_noise(PubArgsPtr R) {
  return Noise<double>{R->qt.q00, R->qt.rr, R->qt.rg, R->qt.rb, R->qt.gg, R->qt.gb, R->qt.bb, R->qt.diag};
}

// NP: adjacent landmark pairs per lane, THREADS: lanes of the workgroup -- <2, 512>: maps up to 2 048 landmarks, one workgroup
// per CU (256 VGPRs); <1, 512>: up to 1 024; <1, 256>: up to 512 landmarks, 143 VGPRs: three workgroups per CU work on three
// particles side by side (the L <= 512 route: what k_step_fused does with a grid walk, a probability queue and seven barriers)
// Which particles a workgroup takes.  The dispatcher deals workgroups round the eight XCDs (workgroup b runs on XCD b mod 8).  After a
// resample the copies of one ancestor stand side by side in the particle order and read the SAME source slot: the publish / subscribe
// kernels let every XCD walk a contiguous EIGHTH of the particles, its 32 workgroups on 32 consecutive particles at a time, so that
// the copies meet in one L2 (4 MB per XCD) -- at the same time, or a turn later -- instead of missing in eight.  A/B on one box
// (profiles/r05/ab_xcd_*.log): k_step_pub, 100 000 x 2 000 in the driver's window: 8.33-8.38 ms (dealt round the XCDs: workgroup b on
// particle b of every turn of 256) -> 8.16-8.18 (the XCD's 32 on consecutive particles of every turn) -> 7.94-7.97 (a contiguous
// eighth).  k_step_pub_big: 20 000 x 5 000 6.18 -> 6.10 ms, a configs[4] shard 40.8 -> 40.8 ms on steps 5-24 and 29.2 -> 28.7 on steps
// 40-49 (runs of 4, 8 or 32 particles of every turn had lost 1-2 % on steps 5-24: ab_big_xcd_runs_4_8.log).
// PK_DIAG_NO_XCD_RUNS: the regression build, the plain deal.
// k_step_pub's walk over the particles [p_begin, p_end): first particle, stride, and where this workgroup's share ends
#ifdef PK_DIAG_NO_XCD_RUNS
__device__ __forceinline__ int64_t pub_walk_first(int64_t p_begin, int64_t) { return p_begin + blockIdx.x; }
__device__ __forceinline__ int64_t pub_walk_stride() { return (int64_t)gridDim.x; }
__device__ __forceinline__ int64_t pub_walk_limit(int64_t, int64_t p_end) { return p_end; }
#else
__device__ __forceinline__ int64_t pub_walk_first(int64_t p_begin, int64_t p_end) {
  const unsigned g = gridDim.x, b = blockIdx.x;
  if ((g & 7u) != 0u) return p_begin + b;
  const int64_t chunk = (p_end - p_begin + 7) / 8;
  return p_begin + (int64_t)(b & 7u) * chunk + (int64_t)(b >> 3);
}
__device__ __forceinline__ int64_t pub_walk_stride() { return (gridDim.x & 7u) != 0u ? (int64_t)gridDim.x : (int64_t)(gridDim.x >> 3); }
__device__ __forceinline__ int64_t pub_walk_limit(int64_t p_begin, int64_t p_end) {
  const unsigned g = gridDim.x, b = blockIdx.x;
  if ((g & 7u) != 0u) return p_end;
  const int64_t chunk = (p_end - p_begin + 7) / 8, e = p_begin + (int64_t)((b & 7u) + 1u) * chunk;
  return e < p_end ? e : p_end;
}
#endif
// TAB (512 lanes only; DESIGN.md section 4, "colour table"): the six colour-covariance rows of a slot are neither read nor written.
// They are a function of (landmark, number of updates) for as long as every map came from one pk_upload_map, and come from the
// table ctab[level][6][Lp] (pk_colour.hpp; L2 hits: a level is 96 KB and the particles sit on a few levels) at the level the
// landmark's count names; k_colour_rows writes them back into slots whenever somebody else wants them.
template <int NP, int THREADS, bool TAB>
__device__ __forceinline__ void step_pub_body() {
  static_assert(!TAB || THREADS == 512, "table mode: the 512-lane instances");
  constexpr int kPubThreads = THREADS, kPubWaves = THREADS / kWave;
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[2][kPubWaves];
  __shared__ int wg_flag[2];
  // Which sixteen landmarks each group of eight lanes works on (<2, 512> only; k_cand_entries, once per scan): the octets with
  // the LONGEST candidate lists go to waves 0-3, the shortest to waves 4-7 -- the waves that come second in the CU's vector
  // memory queue all particle long, and that the others wait for at every barrier
  constexpr bool kPerm = NP == 2 && THREADS == 512;
  __shared__ unsigned short s_perm[kPerm ? 2 * kPubOctets : 1];
  __shared__ unsigned s_rb[kCandSlots];  // the publish table's rank bases (k_cand_entries: entry of (blob g, rank r) = s_rb[r] + g)
  // growing maps: the particle's unmatched blobs, scan order (pub_note_unmatched) -- as many words as the instance's LDS lets a scan have
  // blobs (the 256-lane instance shares a CU with two others: 704 bytes more of static LDS and only two fit -- 0.296 against 0.222 ms)
  constexpr int kUnmWords = THREADS == kPubSmallThreads ? 32 : 96;
  __shared__ unsigned s_ubits[kUnmWords];
  __shared__ unsigned s_kmax;  // TAB: the highest level read so far
  // Lean groups (pub_lean_pair): only this instance deals octets to (wave, pair) groups, and k_cand_entries marks the lean ones for it
#ifdef PK_DIAG_NO_LEAN_BODY  // diagnostic build only: the kernel without the lean body (k_cand_entries ranks and marks as ever)
  constexpr bool kLean = false;
#else
  constexpr bool kLean = kPerm;
#endif
  __shared__ unsigned s_fallbacks;  // kLean: pairs of lean groups that took the usual body after all
  // (the two octet numbers of a lane ride above its index in one register; in a register of their own, or below the index: no
  // better -- profiles/r04/ab_perm_mechanisms.log)
#define PK_PUB_L0(q_, t_) (!kPerm ? 2 * kPubThreads * (q_) + 2 * (t_) : (int)(((lw >> (16 + 8 * (q_))) & 0xFFu) << 4) + 2 * ((t_)&7))
  PubArgsPtr rp = (PubArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const int tid0 = threadIdx.x;
  int B, Lp, L, ecap;
  {
    PubArgsPtr R = pub_args_now(rp);
    if (*R->skip != 0u) return;  // workgroup-uniform: another route takes this scan
    B = R->B;
    Lp = R->Lp;
    L = R->L;
    ecap = R->ecap;
  }
  const unsigned Bp = ((unsigned)B + 15u) & ~15u;
  // LDS offsets (bytes): exact | pub (ecap + 2 entries) | glist (binfo's place) | order | any[2][Bp + 16]
  const unsigned o_pub = Bp * 48u, o_binfo = o_pub + ((unsigned)ecap + 2u) * 8u, o_order = o_binfo + Bp * 4u, o_any = o_order + Bp * 2u;
  const unsigned o_imm = o_any + 2u * (Bp + 16u);
  const unsigned o_bnd = o_imm + (unsigned)kPubImmBytes;  // float2 (Kb, Ib) per landmark
  const unsigned dump = (unsigned)ecap, anydump = Bp;
  unsigned G;  // blobs that several landmarks list
  {
    const int tid = tid0;
    PubArgsPtr R = pub_args_now(rp);
    // ---- the scan's tables: once per workgroup
    {  // the bounds the landmarks' lists were pruned with (no far table: bounds that every landmark meets)
      const uint4* gf = R->far;
      float2* bnd = reinterpret_cast<float2*>(smem + o_bnd);
      for (int i = tid; i < Lp; i += kPubThreads) {
        float2 v = make_float2(-3.0e38f, 0.f);
        if (gf) {
          const uint4 hdr = gf[2 * (size_t)i];
          if (hdr.z != 0u) v = make_float2(__uint_as_float(hdr.x), __uint_as_float(hdr.y));  // (an empty far list: nothing to hold)
        }
        bnd[i] = v;
      }
    }
    double* ex = reinterpret_cast<double*>(smem);
    const double* gex = R->exact;
    for (int i = tid; i < 6 * B; i += kPubThreads) ex[i] = gex[i];
    unsigned* glist = reinterpret_cast<unsigned*>(smem + o_binfo);
    unsigned short* order = reinterpret_cast<unsigned short*>(smem + o_order);
    const unsigned* gb = R->glist;
    const unsigned short* go = R->order;
    G = gb[B];
    for (int i = tid; i < B; i += kPubThreads) {
      glist[i] = (unsigned)i < G ? gb[i] : 0u;
      order[i] = go[i];
    }
    for (unsigned i = (unsigned)tid; i < 2u * (Bp + 16u) / 4u; i += kPubThreads) reinterpret_cast<unsigned*>(smem + o_any)[i] = 0u;
    // the immutable flags (:909, :926): read in the update phase, where a global load would come back behind every store
    // and row request in flight (one in-order vector memory counter)
    const unsigned char* gi = R->immutable;
    for (int i = tid; i < Lp; i += kPubThreads) smem[o_imm + (unsigned)i] = i < L ? gi[i] : (unsigned char)0;
    if constexpr (kPerm) {
      if (tid < 2 * kPubOctets) s_perm[tid] = reinterpret_cast<const unsigned short*>(gb + B + 1)[tid];
    }
    if (tid < kCandSlots) s_rb[tid] = gb[B + 1 + kPubTailWords + tid];
    for (int i = tid; i < kUnmWords; i += kPubThreads) s_ubits[i] = 0u;
    if (tid == 0) {
      wg_flag[0] = 0;
      wg_flag[1] = 0;
      s_kmax = 0u;
      if constexpr (kLean) s_fallbacks = 0u;
    }
  }
  // which of this wave's two groups are lean: bit q = pair q (a scalar; 0 with the switch off)
  unsigned lean_bits = 0u;
  if constexpr (kLean) {
    PubArgsPtr R = pub_args_now(rp);
    if (R->lean != 0) {  // kernel-uniform
      const unsigned m = R->glist[B + 1 + kPubLeanWord], wave = (unsigned)tid0 / kWave;
      lean_bits = __builtin_amdgcn_readfirstlane(((m >> wave) & 1u) | (((m >> (8u + wave)) & 1u) << 1));
    }
  }
  __syncthreads();

  int64_t prev = -1;  // the particle whose partial sums wait in red[] (-1: none, or it went to the general kernels)
  int cur = 0;        // parity of the particle: which any[] / flag / red[] it uses
  // The source slot of the NEXT particle is asked for a whole particle ahead: src[p] is a scalar-cache miss (an L2 round
  // trip) that every row request of the particle depends on (10.8 against 11.2 ms per launch at 100 000 x 2 000).
  int32_t nsrc;
  {
    PubArgsPtr R = pub_args_now(rp);
    const int64_t p0 = pub_walk_first(R->p_begin, R->P), pl = pub_walk_limit(R->p_begin, R->P);
    nsrc = regs_source_pub(R->src, p0 < pl ? p0 : pl - 1);
  }
#ifdef PK_STAMPS
  unsigned long long pst[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
  // the 14 rows + counts of the lane's pair q_ (landmarks lb_, lb_ + 1) of the slot at sslot_
#define PK_PUB_ROW(q_, field, F)                                                                  \
  {                                                                                               \
    const Double2 v_ = *reinterpret_cast<const Double2*>(sf_ + (size_t)F * Lp + lbq_);            \
    S[2 * (q_)].field = v_.x;                                                                     \
    S[2 * (q_) + 1].field = v_.y;                                                                 \
  }
#define PK_PUB_LOAD_MEANS(q_, sslot_, lb_)                                                        \
  {                                                                                               \
    const double* sf_ = reinterpret_cast<const double*>(sslot_);                                  \
    const int lbq_ = (lb_);                                                                       \
    PK_PUB_ROW(q_, mx, F_MX)                                                                      \
    PK_PUB_ROW(q_, my, F_MY)                                                                      \
    PK_PUB_ROW(q_, mr, F_MR)                                                                      \
    PK_PUB_ROW(q_, mg, F_MG)                                                                      \
    PK_PUB_ROW(q_, mb, F_MB)                                                                      \
    asm volatile("" ::: "memory");                                                                \
  }
  // TAB: the pair's counts (asked for ahead of the rows that need them: the level is the table rows' address) ...
#define PK_PUB_LOAD_COUNT(q_, sslot_, coff_, lb_)                                                 \
  {                                                                                               \
    const int* sc_ = reinterpret_cast<const int*>((sslot_) + (coff_));                            \
    const Int2 c_ = *reinterpret_cast<const Int2*>(sc_ + (lb_));                                  \
    S[2 * (q_)].count = c_.x;                                                                     \
    S[2 * (q_) + 1].count = c_.y;                                                                 \
  }
  // ... and its colour blocks from the table, at the levels the counts name.  A level beyond the table (the host leaves the mode
  // before landmarks get there, but runs scans ahead of what it knows: correctness does not rest on it) is reached from the table's
  // last level by the recurrence itself, in a wave-uniform branch -- slow, exact and rare.  The read stays inside the table
  // whatever the count says.
#define PK_PUB_TAB_ROWS(q_, lb_)                                                                  \
  {                                                                                               \
    PubArgsPtr Rt_ = pub_args_now(rp);                                                            \
    const double* tb_ = Rt_->ctab;                                                                \
    const unsigned D_ = (unsigned)Rt_->ctab_depth;                                                \
    const int lbt_ = (lb_);                                                                       \
    bool beyond_ = false;                                                                         \
    _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                            \
      const unsigned k_ = min(colour_level(S[2 * (q_) + j_].count), D_ + kColourBeyondMax);       \
      beyond_ |= k_ >= D_;                                                                        \
      if (k_ > s_kmax) atomicMax(&s_kmax, k_);                                                    \
      /* (a uniform row base and ONE 32-bit byte offset per landmark: the table is below 4 GB -- ct_engage) */ \
      const unsigned bo_ = (min(k_, D_ - 1u) * 6u * (unsigned)Lp + (unsigned)(lbt_ + j_)) * 8u;   \
      const char* tc_ = reinterpret_cast<const char*>(tb_);                                       \
      const size_t rs_ = (size_t)Lp * 8;                                                          \
      S[2 * (q_) + j_].crr = *reinterpret_cast<const double*>(tc_ + bo_);                         \
      S[2 * (q_) + j_].crg = *reinterpret_cast<const double*>(tc_ + rs_ + bo_);                   \
      S[2 * (q_) + j_].crb = *reinterpret_cast<const double*>(tc_ + 2 * rs_ + bo_);               \
      S[2 * (q_) + j_].cgg = *reinterpret_cast<const double*>(tc_ + 3 * rs_ + bo_);               \
      S[2 * (q_) + j_].cgb = *reinterpret_cast<const double*>(tc_ + 4 * rs_ + bo_);               \
      S[2 * (q_) + j_].cbb = *reinterpret_cast<const double*>(tc_ + 5 * rs_ + bo_);               \
    }                                                                                             \
    if (__ballot(beyond_) != 0ull) {                                                              \
      const Noise<double> qtt_ = pub_noise(pub_args_now(rp));                                     \
      _Pragma("unroll 1") for (int j_ = 0; j_ < 2; ++j_) {                                        \
        Landmark<double>& lmt_ = j_ == 0 ? S[2 * (q_)] : S[2 * (q_) + 1];                         \
        const unsigned k_ = min(colour_level(lmt_.count), D_ + kColourBeyondMax);                 \
        Sym3<double> C_{lmt_.crr, lmt_.crg, lmt_.crb, lmt_.cgg, lmt_.cgb, lmt_.cbb};              \
        _Pragma("unroll 1") for (unsigned kk_ = D_ - 1u; kk_ < k_; ++kk_) C_ = colour_block_step(C_, qtt_); \
        lmt_.crr = C_.a;                                                                          \
        lmt_.crg = C_.b;                                                                          \
        lmt_.crb = C_.c;                                                                          \
        lmt_.cgg = C_.d;                                                                          \
        lmt_.cgb = C_.e;                                                                          \
        lmt_.cbb = C_.f;                                                                          \
      }                                                                                           \
    }                                                                                             \
    asm volatile("" ::: "memory");                                                                \
  }
  // (TAB: the counts came with PK_PUB_LOAD_COUNT)
#define PK_PUB_LOAD_COVS(q_, sslot_, coff_, lb_)                                                  \
  {                                                                                               \
    const double* sf_ = reinterpret_cast<const double*>(sslot_);                                  \
    const int lbq_ = (lb_);                                                                       \
    PK_PUB_ROW(q_, pxx, F_PXX)                                                                    \
    PK_PUB_ROW(q_, pxy, F_PXY)                                                                    \
    PK_PUB_ROW(q_, pyy, F_PYY)                                                                    \
    if constexpr (!TAB) {                                                                         \
      const int* sc_ = reinterpret_cast<const int*>((sslot_) + (coff_));                          \
      PK_PUB_ROW(q_, crr, F_CRR)                                                                  \
      PK_PUB_ROW(q_, crg, F_CRG)                                                                  \
      PK_PUB_ROW(q_, crb, F_CRB)                                                                  \
      PK_PUB_ROW(q_, cgg, F_CGG)                                                                  \
      PK_PUB_ROW(q_, cgb, F_CGB)                                                                  \
      PK_PUB_ROW(q_, cbb, F_CBB)                                                                  \
      const Int2 c_ = *reinterpret_cast<const Int2*>(sc_ + lbq_);                                 \
      S[2 * (q_)].count = c_.x;                                                                   \
      S[2 * (q_) + 1].count = c_.y;                                                               \
      asm volatile("" ::: "memory");                                                              \
    } else {                                                                                      \
      PK_PUB_TAB_ROWS(q_, lbq_)                                                                   \
    }                                                                                             \
  }
  // (TAB: counts first, no colour rows -- PK_PUB_TAB_ROWS follows at the top of the particle, when the counts have long arrived)
#define PK_PUB_LOAD_PAIR(q_, sslot_, coff_, lb_)                                                  \
  {                                                                                               \
    const double* sf_ = reinterpret_cast<const double*>(sslot_);                                  \
    const int* sc_ = reinterpret_cast<const int*>((sslot_) + (coff_));                            \
    const int lbq_ = (lb_);                                                                       \
    if constexpr (TAB) {                                                                          \
      const Int2 c_ = *reinterpret_cast<const Int2*>(sc_ + lbq_);                                 \
      S[2 * (q_)].count = c_.x;                                                                   \
      S[2 * (q_) + 1].count = c_.y;                                                               \
    }                                                                                             \
    PK_PUB_ROW(q_, mx, F_MX)                                                                      \
    PK_PUB_ROW(q_, my, F_MY)                                                                      \
    PK_PUB_ROW(q_, mr, F_MR)                                                                      \
    PK_PUB_ROW(q_, mg, F_MG)                                                                      \
    PK_PUB_ROW(q_, mb, F_MB)                                                                      \
    asm volatile("" ::: "memory");                                                                \
    PK_PUB_ROW(q_, pxx, F_PXX)                                                                    \
    PK_PUB_ROW(q_, pxy, F_PXY)                                                                    \
    PK_PUB_ROW(q_, pyy, F_PYY)                                                                    \
    if constexpr (!TAB) {                                                                         \
      PK_PUB_ROW(q_, crr, F_CRR)                                                                  \
      PK_PUB_ROW(q_, crg, F_CRG)                                                                  \
      PK_PUB_ROW(q_, crb, F_CRB)                                                                  \
      PK_PUB_ROW(q_, cgg, F_CGG)                                                                  \
      PK_PUB_ROW(q_, cgb, F_CGB)                                                                  \
      PK_PUB_ROW(q_, cbb, F_CBB)                                                                  \
      const Int2 c_ = *reinterpret_cast<const Int2*>(sc_ + lbq_);                                 \
      S[2 * (q_)].count = c_.x;                                                                   \
      S[2 * (q_) + 1].count = c_.y;                                                               \
    }                                                                                             \
    asm volatile("" ::: "memory");                                                                \
  }
  // The lane's FIRST pair of the next particle is asked for as soon as this particle's first pair has been stored -- into
  // the registers that store has just freed -- so its rows fly while the second pair is updated and stored.
  Landmark<double> S[2 * NP];
  constexpr int kPipe = 1;  // pairs asked for ahead (both: 58 registers spilled)
  // the lane's index and (kPerm) the octets of its two pairs in one register: tid | octet of pair 0 << 16 | of pair 1 << 24
  // (0xFF: none, the lane is beyond the map) -- read from LDS at every use the table cost 1.3 % of the kernel's time
  unsigned lane_word = (unsigned)tid0;
  if constexpr (kPerm) {
    const unsigned octs = (unsigned)(s_perm[tid0 >> 3] & 0xFFu) | ((unsigned)(s_perm[kPubOctets + (tid0 >> 3)] & 0xFFu) << 8);
    lane_word = (unsigned)tid0 | (octs << 16);
  }
  {
    const unsigned lw = lane_word;
    PubArgsPtr R = pub_args_now(rp);
    const unsigned char* ns = pub_slot_source(R).at(nsrc);
    const int coff = R->count_off;
#pragma unroll
    for (int q = 0; q < kPipe; ++q) PK_PUB_LOAD_PAIR(q, ns, coff, min(PK_PUB_L0(q, tid0), Lp - 2))
  }
  for (int64_t p = pub_walk_first(pub_args_now(rp)->p_begin, pub_args_now(rp)->P);; p += pub_walk_stride(), cur ^= 1) {
    // everything derived from the lane index is derived afresh for every particle (hoisted out of the loop those values
    // occupy registers for the whole kernel)
    unsigned lw = lane_word;
    asm volatile("" : "+v"(lw));
    int tid;
    if constexpr (!kPerm) {
      tid = (int)lw;
    } else {
      tid = (int)(lw & 0xFFFFu);
    }
    double* ex = reinterpret_cast<double*>(smem);
    double* pub = reinterpret_cast<double*>(smem + o_pub);
    const unsigned* glist = reinterpret_cast<const unsigned*>(smem + o_binfo);
    const unsigned short* order = reinterpret_cast<const unsigned short*>(smem + o_order);
    unsigned char* anyc = smem + o_any + (unsigned)cur * (Bp + 16u);
    PubSlots Q[2 * NP];
    double pse[2 * NP];
    bool done;
    unsigned lean_ok = 0u;  // (wave-uniform) bit q: pair q went through the lean body -- its take bits are set, pub_take has nothing to add
    PK_STAMP(s0)
#ifdef PK_STAMPS
    unsigned long long s3 = s0;
#endif
    {
      // (no branch on `done` in front of the requests: every kernel argument they need comes in one batch; a workgroup
      // that has run out of particles asks for the last particle's rows once more and drops them)
      PubArgsPtr R = pub_args_now(rp);
      const int64_t Pn = pub_walk_limit(R->p_begin, R->P);
      done = p >= Pn;
      const int64_t pc = done ? Pn - 1 : p;
      {
        const SlotSource ss = pub_slot_source(R);
        const unsigned char* sslot = ss.at(nsrc);
        const double sx = pose_scalar(R->x, pc), sy = pose_scalar(R->y, pc), sh = pose_scalar(R->h, pc);
        // the lane's landmarks: pair q = landmarks 1024 q + 2 tid, + 1 (lanes beyond the map re-read its last pair and
        // never use or store it)
        int lbase[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) lbase[q] = min(PK_PUB_L0(q, tid), Lp - 2);
        // ---- 1. requests: candidate records (L2), the means of all four landmarks, then the covariance rows
        // (the first pair's now, in front of the rows; the second pair's behind the first pair's verdicts -- by then every row has
        // arrived, and twelve registers fewer are live while the verdicts are worked out)
        uint4 cref[2 * NP], ccw[2 * NP], cew[2 * NP];
        auto request_cand = [&](int q) {
          PubArgsPtr R2 = pub_args_now(rp);
          // (lanes beyond the map: the spare records behind the table, whose lists are empty -- the ROWS such a lane holds are
          // the last pair's once more, and with that pair's lists it would gate, take and weigh the pair's blobs a second time)
#ifdef PK_DIAG_TAIL_LISTS  // diagnostic build only: round 3's indexing, to show that the regression test bites
          const int lc = lbase[q];
#else
          const int lc = min(PK_PUB_L0(q, tid), Lp);
#endif
          const uint4* cr = R2->cand + 2 * (size_t)lc;
          const uint4* er = R2->erec + lc;
          cref[2 * q] = cr[0];
          ccw[2 * q] = cr[1];
          cref[2 * q + 1] = cr[2];
          ccw[2 * q + 1] = cr[3];
          cew[2 * q] = er[0];
          cew[2 * q + 1] = er[1];
        };
        request_cand(0);
        asm volatile("" ::: "memory");
        if constexpr (TAB) {  // the first pair's colour blocks (its counts came a particle ago)
          static_assert(kPipe == 1, "the pairs asked for ahead take their table rows here");
          PK_PUB_TAB_ROWS(0, lbase[0])
        }
        // (pair by pair, means before covariance rows: the first pair's gates and verdicts are worked out while the second
        // pair's rows are still on their way -- the vector memory counter retires in order)
        {  // the next particle's source slot (pinned here: the wait for it passes under the wait for the first rows)
          PubArgsPtr R4 = pub_args_now(rp);
          const int64_t pn = p + pub_walk_stride(), pl = pub_walk_limit(R4->p_begin, R4->P);
          nsrc = regs_source_pub(R4->src, pn < pl ? pn : pl - 1);
          asm volatile("" : "+s"(nsrc));
        }
        PK_STAMP(s1)
        PK_PSTAMP(0, s0, s1)  // scalars, requests
        // ---- 2. per pair: gates of its two landmarks (means only; failing candidates published at once), then their verdicts
        // on the gate-passing blobs (first use of the covariance rows)
        // (written out per pair: as nested unrolled loops the slot words were not promoted to registers)
        auto do_pair = [&](auto qc) {
          constexpr int q = decltype(qc)::value;

    const int l0 = PK_PUB_L0(q, tid);
    const PubGateIn gi[2] = {{cref[2 * q], {ccw[2 * q], ccw[2 * q]}, {cew[2 * q], cew[2 * q]}, S[2 * q].mx, S[2 * q].my,
                              S[2 * q].mr, S[2 * q].mg, S[2 * q].mb, l0 < L},
                             {cref[2 * q + 1], {ccw[2 * q + 1], ccw[2 * q + 1]}, {cew[2 * q + 1], cew[2 * q + 1]},
                              S[2 * q + 1].mx, S[2 * q + 1].my, S[2 * q + 1].mr, S[2 * q + 1].mg, S[2 * q + 1].mb,
                              l0 + 1 < L}};
    PubSlots qq[2] = {kPubNoSlots,
                      kPubNoSlots};
    double pp[2] = {0.0, 0.0};
    if constexpr (THREADS == kPubSmallThreads) { /* three workgroups per CU: one landmark at a time (168 VGPRs) */
      
#pragma unroll
      for (int j_ = 0; j_ < 2; ++j_) {
        const PubGateIn g1[1] = {gi[j_]};
        PubSlots q1[1] = {qq[j_]};
        double p1[1] = {0.0};
        const Landmark<double>* const l1[1] = {&S[2 * q + j_]};
        if (PK_PUB_ABLATE < 4) pub_gatesN<1>(q1, p1, g1, ex, pub, dump, &wg_flag[cur], sx, sy, sh);
        if (PK_PUB_ABLATE < 3) {
          struct Chk1 {
            const float2* bnd_;
            int l_, L_, Lp_;
            PubArgsPtr rp_;
            double sh;
            __device__ __forceinline__ float2 bnd(int) const { return bnd_[min(l_, Lp_ - 1)]; }
            __device__ __forceinline__ bool has(int) const { return l_ < L_; }
            __device__ __forceinline__ const uint4* far_row() const {
              const uint4* fr = pub_args_now(rp_)->far;
              return fr ? fr + 2 * (size_t)min(l_, Lp_) : nullptr;
            }
          };
          const Chk1 chk{reinterpret_cast<const float2*>(smem + o_bnd), l0 + j_, L, Lp, rp, sh};
          pub_keysN<1, kPubSlots, false, true, 1, Chk1>(q1, l1, p1, ex, pub, dump, anyc, anydump, &wg_flag[cur], sx, sy, nullptr, nullptr, chk);
        }
        qq[j_] = q1[0];
        pp[j_] = p1[0];
      }
    } else {
      const Landmark<double>* const l2[2] = {&S[2 * q], &S[2 * q + 1]};
      bool usual = true;  // wave-uniform
      if constexpr (kLean) {
        if (((lean_bits >> q) & 1u) != 0u && PK_PUB_ABLATE == 0) {
          const float2* bt = reinterpret_cast<const float2*>(smem + o_bnd);
          const float2 b2[2] = {bt[min(l0, Lp - 1)], bt[min(l0 + 1, Lp - 1)]};
          usual = !pub_lean_pair(qq, pp, gi, l2, b2, ex, anyc, anydump, sx, sy, sh);
          lean_ok |= usual ? 0u : (1u << q);
          if (usual && (tid & (kWave - 1)) == 0) atomicAdd(&s_fallbacks, 1u);
        }
      }
      if (usual) {
      if (PK_PUB_ABLATE < 4) pub_gatesN<2, 1, kPubSlots, true>(qq, pp, gi, ex, pub, dump, &wg_flag[cur], sx, sy, sh);
      PK_STAMP(sk0_)
      if (PK_PUB_ABLATE < 3) {
        /* (the landmarks' own far bounds are held against the ones the scan's lists were pruned with: pub_far_recheck) */
        struct Chk2 {
          const float2* bnd_;
          unsigned lw, tid_;
          int L_, Lp_;
          PubArgsPtr rp_;
          double sh;
          __device__ __forceinline__ int l0() const { const unsigned lw = this->lw; const int tid = (int)tid_; (void)tid; return PK_PUB_L0(q, tid); }
          __device__ __forceinline__ float2 bnd(int j) const { return bnd_[min(l0() + j, Lp_ - 1)]; }
          __device__ __forceinline__ bool has(int j) const { return l0() + j < L_; }
          __device__ __forceinline__ const uint4* far_row() const {
            const uint4* fr = pub_args_now(rp_)->far;
            return fr ? fr + 2 * (size_t)min(l0(), Lp_) : nullptr;
          }
        };
        const Chk2 chk{reinterpret_cast<const float2*>(smem + o_bnd), lw, (unsigned)tid, L, Lp, rp, sh};
        pub_keysN<2, kPubSlots, false, true, 1, Chk2>(qq, l2, pp, ex, pub, dump, anyc, anydump, &wg_flag[cur], sx, sy, nullptr, nullptr, chk);
        { /* (a second turn where a landmark passed more blobs than it has slots: wave-uniform, rare) */
          PubArgsPtr R9 = pub_args_now(rp);
          const int lc9 = min(l0, Lp);
          if (pub_refill_slots<2>(qq, R9->cand + 2 * (size_t)lc9, R9->erec + lc9, &wg_flag[cur]))
            pub_keysN<2>(qq, l2, pp, ex, pub, dump, anyc, anydump, &wg_flag[cur], sx, sy);
        }
      }
      PK_STAMP(sk1_)
      PK_PSTAMP(2, sk0_, sk1_) /* keys: part of the gates-and-verdicts slot */
      }
    }
    Q[2 * q] = qq[0];
    Q[2 * q + 1] = qq[1];
    pse[2 * q] = pp[0];
    pse[2 * q + 1] = pp[1];
  
        };
        if (!done) {  // workgroup-uniform
          do_pair(std::integral_constant<int, 0>{});
          if constexpr (NP > 1) {
            // The SECOND pair's rows are asked for HERE -- behind the first pair's keys, its five mean rows in front of its
            // candidate records (its gates need both at once), the other rows behind them: the texture addresser takes a CU's
            // vector-memory instructions in order, ~16 cycles per 1 KB; at the top of the particle these fifteen requests of each of
            // the eight waves stood between the last row stores and what the first gates need at once, and the rows still arrive
            // long before the second pair's gates are through their atan2.  At the top: 9.96 ms per step; behind the first pair's
            // gates 9.83; behind its keys 9.71; here 9.465 (profiles/r04/ab_second_pair_rows_later.log, ab_request_order_*.log).
            if constexpr (TAB) {  // (first in its batch: the table rows below wait for it, and with it for everything asked for before it)
              PubArgsPtr R8 = pub_args_now(rp);
              PK_PUB_LOAD_COUNT(1, sslot, R8->count_off, lbase[1])
              asm volatile("" ::: "memory");
            }
            PK_PUB_LOAD_MEANS(1, sslot, lbase[1])
            request_cand(NP - 1);
            {
              asm volatile("" ::: "memory");
              PubArgsPtr R7 = pub_args_now(rp);
              PK_PUB_LOAD_COVS(1, sslot, R7->count_off, lbase[1])
            }
            do_pair(std::integral_constant<int, 1>{});
            if constexpr (TAB) {
              // (the first pair's colour blocks were let go behind its verdicts -- 24 registers the second pair's verdicts need -- and
              // come once more from the table, L2 hits that land while the barriers and the settling pass)
              PK_PUB_TAB_ROWS(0, lbase[0])
            }
          }
        }
        PK_STAMP(s2)
        PK_PSTAMP(1, s1, s2)  // gates and verdicts
#ifdef PK_STAMPS
        s3 = s2;
#endif
      }
    }
    lds_barrier();  // A: every verdict of this particle is in the table
    PK_STAMP(s4)
    PK_PSTAMP(3, s3, s4)  // barrier A
    if (prev >= 0 && tid == 0) {  // the previous particle's log-weight (its partial sums were written before A)
      PubArgsPtr R = pub_args_now(rp);
      double tot = red[cur ^ 1][0];
#pragma unroll
      for (int i = 1; i < kPubWaves; ++i) tot += red[cur ^ 1][i];
      double* logw = R->logw;
      const double w = (R->reset ? 0.0 : logw[prev]) + tot;
      logw[prev] = w;
      unsigned long long* gk = R->gmax_key;
      if (gk) atomicMax(gk + (prev & (kGmaxKeys - 1)), double_to_key(w));
      R->src[prev] = (int32_t)prev;
    }
    if (done) break;
    prev = -1;
    // ---- 4. settling, one lane per contested blob; blobs nobody matches; the next particle's any[] / flag cleared
    double acc;
    {
      int nun = 0;
      for (unsigned w = (unsigned)tid; w < Bp / 4u; w += kPubThreads) {
        const unsigned v = reinterpret_cast<const unsigned*>(anyc)[w];
#pragma unroll
        for (int b = 0; b < 4; ++b) nun += ((int)(4 * w + b) < B && ((v >> (8 * b)) & 0xFFu) == 0u) ? 1 : 0;
      }
      acc = (double)nun * Consts<double>::log_no_match;  // unseen features: weight *= 0.1 each (:94-95)
      unsigned* anyn = reinterpret_cast<unsigned*>(smem + o_any + (unsigned)(cur ^ 1) * (Bp + 16u));
      for (unsigned w = (unsigned)tid; w < Bp / 4u; w += kPubThreads) anyn[w] = 0u;
      if (tid == 0) wg_flag[cur ^ 1] = 0;
    }
    if (pub_args_now(rp)->unm != nullptr) pub_note_unmatched<THREADS>(tid, anyc, order, B, Bp, s_ubits);  // kernel-uniform: growing maps only
    if (PK_PUB_ABLATE < 2) pub_settle_blobs<THREADS>(tid, glist, G, pub, dump, &wg_flag[cur], s_rb);
    PK_STAMP(s5)
    PK_PSTAMP(4, s4, s5)  // unseen blobs, settling
    lds_barrier();  // B: every winner is marked, every flag is set
    {
      PubArgsPtr Ru = pub_args_now(rp);
      if (Ru->unm != nullptr) pub_store_unmatched<THREADS>(tid, s_ubits, Ru->unm + (size_t)p * Ru->unm_words, Ru->unm_words);
    }
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i)
      if (PK_PUB_ABLATE < 2 && (!kLean || ((lean_ok >> (i / 2)) & 1u) == 0u)) pub_take(Q[i], pub, dump);
    lds_barrier();  // C: every marker has been read -- the table is the next particle's
    PK_STAMP(s6)
    PK_PSTAMP(5, s5, s6)  // barrier B, markers, barrier C
    if (wg_flag[cur] && PK_PUB_ABLATE == 0) {  // workgroup-uniform: nothing has been written; the general kernels take the particle
      if (tid == 0) {
        PubArgsPtr R = pub_args_now(rp);
        R->pflag_out[p] = 1;
        atomicAdd(R->n_flagged, 1u);
      }
      {  // (the next particle's first pair is asked for on this way out as well)
        PubArgsPtr R6 = pub_args_now(rp);
        const unsigned char* ns = pub_slot_source(R6).at(nsrc);
        const int coff = R6->count_off;
#pragma unroll
        for (int q = 0; q < kPipe; ++q) PK_PUB_LOAD_PAIR(q, ns, coff, min(PK_PUB_L0(q, tid), Lp - 2))
      }
      continue;
    }
    // ---- 5. updates in scan order, stores
    {
      PubArgsPtr R = pub_args_now(rp);
      if (tid == 0) R->pflag_out[p] = 0;
      const Noise<double> qt = pub_noise(R);
      const double sx = pose_scalar(R->x, p), sy = pose_scalar(R->y, p);
      unsigned char* dslot = R->map_dst + (size_t)p * R->ss.slot_bytes;
      double* df = reinterpret_cast<double*>(dslot);
      int* dc = reinterpret_cast<int*>(dslot + R->count_off);
      const unsigned char* immutable = smem + o_imm;
      {  // a pair's rows go out behind both its updates.  (Measured and dropped, round 4: the update of a pair in halves -- position
        // blocks, five rows out, colour blocks, nine rows out: +0.5 %, ab_update_in_halves.log; pair 0's rows out between pair 1's
        // updates, a third or a half at a time: +3.3 % / +7.2 %, ab_atan2_fmak_interleaved_stores.log; the two halves of the workgroup
        // out of step: +3 % / +0.5 %, ab_update_phase_as_lambdas_and_staggered_halves.log; wave priorities: ab_wave_priorities.log.)
        // do_apply(q): the pair's two updates; do_store(q): its rows out and -- q < kPipe -- the next particle's pair asked for into
        // the registers just stored
        double nprod = 1.0;  // (the product of the norms of this lane's updates: pub_fold_norms)
        auto do_apply = [&](auto qc) {
          constexpr int q = decltype(qc)::value;
          const int l0 = PK_PUB_L0(q, tid);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int i = 2 * q + j;
            const bool imm = immutable[min(l0 + j, Lp - 1)] != 0;
            if (PK_PUB_ABLATE < 1)
              acc += THREADS == kPubSmallThreads ? pub_apply_loop(Q[i], ex, order, qt, S[i], imm, sx, sy, pse[i], nullptr, 0, 0, 0xFFFFu, PK_PROD_PTR(nprod))
                                                 : pub_apply<TAB>(Q[i], ex, order, qt, S[i], imm, sx, sy, pse[i], PK_PROD_PTR(nprod));
          }
          if constexpr (q == NP - 1) pub_fold_norms(acc, nprod);
        };
        auto do_store = [&](auto qc) {
          constexpr int q = decltype(qc)::value;
          const int l0 = PK_PUB_L0(q, tid);
          PK_STAMP(su0_)
          if (l0 < Lp) {
            // (non-temporal: nothing reads the rows before the next step; sc1 or plain stores 11.45, 11.65 against 11.05 ms, round 3)
#define PK_PUB_STORE(field, F)                                                             \
    {                                                                                        \
      const Double2 v = {S[2 * q].field, S[2 * q + 1].field};                                \
      __builtin_nontemporal_store(v, reinterpret_cast<Double2*>(df + (size_t)F * Lp + l0)); \
    }
            PK_PUB_STORE(mx, F_MX)
            PK_PUB_STORE(my, F_MY)
            PK_PUB_STORE(mr, F_MR)
            PK_PUB_STORE(mg, F_MG)
            PK_PUB_STORE(mb, F_MB)
            PK_PUB_STORE(pxx, F_PXX)
            PK_PUB_STORE(pxy, F_PXY)
            PK_PUB_STORE(pyy, F_PYY)
            if constexpr (!TAB) {
              PK_PUB_STORE(crr, F_CRR)
              PK_PUB_STORE(crg, F_CRG)
              PK_PUB_STORE(crb, F_CRB)
              PK_PUB_STORE(cgg, F_CGG)
              PK_PUB_STORE(cgb, F_CGB)
              PK_PUB_STORE(cbb, F_CBB)
            }
#undef PK_PUB_STORE
            const Int2 c = {S[2 * q].count, S[2 * q + 1].count};
            __builtin_nontemporal_store(c, reinterpret_cast<Int2*>(dc + l0));
          }
          if (q < kPipe) {  // the next particle's pair, into the registers just stored (asked for later: +9 %, ab_request_order_more.log)
            PubArgsPtr R6 = pub_args_now(rp);
            const unsigned char* ns = pub_slot_source(R6).at(nsrc);
            PK_PUB_LOAD_PAIR(q, ns, R6->count_off, min(PK_PUB_L0(q, tid), Lp - 2))
          }
          PK_STAMP(su1_)
          PK_PSTAMP(10, su0_, su1_)  // of the updates: rows out, the next particle's first pair asked for
        };
        using Q0 = std::integral_constant<int, 0>;
        using Q1 = std::integral_constant<int, 1>;
        do_apply(Q0{});
        do_store(Q0{});
        if constexpr (NP == 2) {
          do_apply(Q1{});
          do_store(Q1{});
        }
      }
    }
    PK_STAMP(s7)
    PK_PSTAMP(6, s6, s7)  // updates, stores issued
    {
      const double ws = wave_sum(acc);  // the sum over the workgroup is finished behind the next barrier A
      if ((tid & (kWave - 1)) == 0) red[cur][tid / kWave] = ws;
      prev = p;
    }
    PK_STAMP(s8)
    PK_PSTAMP(7, s7, s8)  // wave sum
    PK_PSTAMP(8, s0, s8)  // particle
#ifdef PK_STAMPS
    pst[9] += 1ull;
#endif
  }
#ifdef PK_STAMPS
  if ((tid0 & 63) == 0)
    for (int k = 0; k < 12; ++k) {
      atomicAdd(&pk_pstamp_acc[k], pst[k]);
      if (THREADS == 512) atomicAdd(&pk_pstamp_wave[tid0 >> 6][k], pst[k]);
    }
#endif
  if constexpr (TAB) {  // (behind the last barrier A: every lane's level is in)
    if (tid0 == 0) atomicMax(pub_args_now(rp)->ctab_max, s_kmax);
  }
  if constexpr (kLean) {  // (likewise: every fallback was counted in front of a barrier A)
    if (tid0 == 0 && s_fallbacks != 0u) {
      unsigned* st = const_cast<unsigned*>((const unsigned*)pub_args_now(rp)->stats);
      if (st) atomicAdd(st + 6, s_fallbacks);
    }
  }
}
template <int NP, int THREADS>
__global__ void __launch_bounds__(THREADS, THREADS == 256 ? 3 : 1) k_step_pub(PubArgs a_unused) {
  step_pub_body<NP, THREADS, false>();
}
template <int NP, int THREADS, bool TAB>
__global__ void __launch_bounds__(THREADS, 1) k_step_pub(PubArgs a_unused) {
  static_assert(TAB, "the plain instances are k_step_pub<NP, THREADS>");
  step_pub_body<NP, THREADS, true>();
}

// ------------------------------------------------------------------ maps beyond 2 048 landmarks: the same, in two passes
// A particle of 5 000 landmarks is 1.16 MB of state: it fits neither the CU's registers nor its LDS, so the map cannot stay
// on chip between the verdicts and the updates.  k_step_pub_big walks the map twice, pair by pair (1 024 landmarks a turn):
//   pass 1  rows in -> gates -> verdicts published -- the rows are dropped, what stays in registers is the seven words per
//           landmark the second pass needs (the gate-passing blobs with their entries, the expected bearing);
//   barriers, blob-parallel settling, markers (as in k_step_pub);
//   pass 2  back to front: the last pair's rows are still in the registers, the others come in again (L2 / Infinity Cache: the same
//           workgroup read them microseconds ago) -> updates -> rows out.
// HBM sees the state once on the way in (the second read is a cache hit, which the FETCH_SIZE counter still counts) and once
// on the way out.  The scan's exact records (48 B x B: 240 KB at 5 000 blobs) do not fit LDS beside the publish table; they
// are read from L2.  Candidate and inverse lists of sixteen entries (eight overflow somewhere in every scan of several
// thousand blobs).  NCH: pairs per lane, Lp <= 1 024 NCH.
constexpr int kPubBigSlots = 2 * kCandSlots;
// Gate-passing blobs a landmark may have in pass 1: among several thousand random colours some landmark of every particle
// passes five to seven.  Only those with a probability > 0 -- once the colour blocks have tightened,
// the landmark's own blob and the odd look-alike -- are carried to pass 2, at most kPubSlots of them.
constexpr int kPubBigGateSlots = 8;
__device__ __forceinline__ PubSlots pub_keep_positive(const PubSlotsT<kPubBigGateSlots>& g, int* flag) {
  PubSlots o = kPubNoSlots;
#pragma unroll
  for (int k = kPubBigGateSlots - 1; k >= 0; --k) {  // (back to front: the order of the slots is kept)
    const bool pos = ((g.st >> (4 * k)) & 1u) != 0u;
    o.s[3] = pos ? o.s[2] : o.s[3];
    o.s[2] = pos ? o.s[1] : o.s[2];
    o.s[1] = pos ? o.s[0] : o.s[1];
    o.s[0] = pos ? g.s[k] : o.s[0];
    o.st = pos ? ((o.st << 4) | 1u) : o.st;
  }
  if (flag && __popc(g.st & 0x11111111u) > kPubSlots) *flag = 1;
  o.st &= 0xFFFFu;  // (a state nibble per blob of probability > 0 was shifted in: only the four kept ones' stay -- the upper half is
                    // where pub_park_beyond_four puts the place of the others)
  return o;
}
// Round 6: a landmark with MORE than four blobs of probability > 0 -- on the first scan of a fresh map of several thousand landmarks
// (0.25 I colour blocks: every look-alike inside the gates counts) a hundred landmarks of EVERY particle, so that every particle of
// step 0 was handed to the fall-back kernels: 115 ms where the steps behind it take 7 (20 000 x 5 000), 0.7 s at a configs[4] shard --
// keeps its first four in the slots as before and parks the fifth to eighth in LDS: the entries of the publish table this scan does
// not use (k_cand_entries' figure says how many it does) are the overflow area, 16 bytes a place, dealt out by a counter.  Behind
// the settling the landmark looks at the parked blobs' markers too; a parked blob it TAKES moves into a slot it did not take (there
// nearly always is one: a landmark takes one blob, rarely two); only a landmark that takes more than four sends the particle on.
__device__ __forceinline__ uint4 pub_positive_beyond_four(const PubSlotsT<kPubBigGateSlots>& g) {
  unsigned x[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  int c = 0;
#pragma unroll
  for (int k = 0; k < kPubBigGateSlots; ++k) {
    const bool pos = ((g.st >> (4 * k)) & 1u) != 0u;
    x[0] = (pos && c == 4) ? g.s[k] : x[0];
    x[1] = (pos && c == 5) ? g.s[k] : x[1];
    x[2] = (pos && c == 6) ? g.s[k] : x[2];
    x[3] = (pos && c == 7) ? g.s[k] : x[3];
    c += pos ? 1 : 0;
  }
  return make_uint4(x[0], x[1], x[2], x[3]);
}
// ... in pass 1: the place goes into the upper half of the slots' state word (place + 1; 0: nothing parked)
__device__ __forceinline__ void pub_park_beyond_four(PubSlots& q, const PubSlotsT<kPubBigGateSlots>& g, uint4* ovf, unsigned n_places, unsigned* counter,
                                                     int* flag) {
  if (__popc(g.st & 0x11111111u) > kPubSlots) {
    const unsigned place = atomicAdd(counter, 1u);
    if (place < n_places) {
      ovf[place] = pub_positive_beyond_four(g);
      q.st |= (place + 1u) << 16;
    } else {
      *flag = 1;
    }
  }
}
// ... behind the settling (after pub_take): the parked blobs this landmark takes move into slots it did not take
__device__ __forceinline__ void pub_take_parked(PubSlots& q, const uint4* ovf, const double* pub, unsigned dump, int* flag) {
  const unsigned pl = q.st >> 16;
  if (__ballot(pl != 0u) == 0ull) return;  // wave-uniform: the usual case
  if (pl != 0u) {
    const uint4 s4 = ovf[pl - 1u];
    const unsigned xw[4] = {s4.x, s4.y, s4.z, s4.w};
    double m[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const unsigned e = xw[x] >> 16;
      m[x] = pub[e == 0xFFFFu ? dump : e];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const unsigned e = xw[x] >> 16;
      const bool take = (xw[x] & 0xFFFFu) != 0xFFFFu && (e == 0xFFFFu || m[x] == pub_marker());  // (every parked blob has probability > 0)
      bool placed = !take;
#pragma unroll
      for (int sidx = 0; sidx < kPubSlots; ++sidx) {
        const bool here = !placed && ((q.st >> (4 * sidx)) & 4u) == 0u;
        q.s[sidx] = here ? xw[x] : q.s[sidx];
        q.st = here ? ((q.st & ~(0xFu << (4 * sidx))) | (5u << (4 * sidx))) : q.st;
        placed |= here;
      }
      if (!placed) *flag = 1;  // more than four blobs taken: the fall-back kernels
    }
  }
  q.st &= 0xFFFFu;
}
// (at B = 5 000 the publish table needs some 15 000 entries: the scan-order table -- read only where a landmark takes two
// blobs -- stays in global memory, and there is no room for the immutable flags either)
__host__ __device__ inline size_t pub_big_fixed_lds_bytes(int B) {
  const size_t Bp = ((size_t)B + 15) & ~(size_t)15;
  return 16 + Bp * 4 + 2 * (Bp + 16);
}
int step_pub_big_entry_capacity(int B) {
  const size_t fixed = pub_big_fixed_lds_bytes(B);
  if (fixed + 64 * 8 > kMaxDynLds) return 0;
  const size_t e = (kMaxDynLds - fixed) / 8;
  return (int)(e > 65534 ? 65534 : e);
}
size_t step_pub_big_lds_bytes(int B, int ecap) { return pub_big_fixed_lds_bytes(B) + (size_t)ecap * 8; }

// (k_step_pub's walk: a contiguous eighth of the particles per XCD)
#define PK_BIG_FIRST(R_) pub_walk_first((R_)->p_begin, (R_)->P)
#define PK_BIG_STRIDE() pub_walk_stride()
#define PK_BIG_LIMIT(R_) pub_walk_limit((R_)->p_begin, (R_)->P)
template <int NCH>
__global__ void __launch_bounds__(kPubThreads) k_step_pub_big(PubArgs a_unused) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[2][kPubThreads / kWave];
  __shared__ int wg_flag[2];
  // which sixteen landmarks the eight lanes of place 64 q + tid / 8 work on in chunk q (k_cand_entries: the octets ranked by
  // their longest candidate list, so that a wave's -- and a chunk's -- lists are of like length)
  __shared__ unsigned short s_bperm[kPubBigPlaces];
  __shared__ unsigned s_rb[kPubBigSlots];  // the publish table's rank bases (k_cand_entries)
  __shared__ unsigned s_novf[2];           // places of the overflow area dealt out in pass 1 to the particle of either parity (pub_park_beyond_four)
  __shared__ unsigned s_ubits[kPubUnmWords];  // growing maps: the particle's unmatched blobs, scan order (pub_note_unmatched)
#define PK_BIG_L0(q_, t_) ((int)(16u * (unsigned)s_bperm[kPubOctets * (q_) + ((t_) >> 3)]) + 2 * ((t_)&7))
  constexpr int kPubWaves = kPubThreads / kWave;
#ifdef PK_DIAG_BIG_FRONT_TO_BACK  // (regression build: pass 2 front to back from rows asked for again, as until round 5)
  constexpr bool kBack = false;
#else
  constexpr bool kBack = NCH < 6;  // pass 2 back to front, from the pair pass 1 ended on (see below)
#endif
  PubArgsPtr rp = (PubArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const int tid0 = threadIdx.x;
  int B, Lp, L, ecap;
  {
    PubArgsPtr R = pub_args_now(rp);
    if (*R->skip != 0u) return;  // workgroup-uniform: another route takes this scan
    B = R->B;
    Lp = R->Lp;
    L = R->L;
    ecap = R->ecap;
  }
  const unsigned Bp = ((unsigned)B + 15u) & ~15u;
  // LDS offsets (bytes): pub (ecap + 2 entries) | glist | any[2][Bp + 16]
  const unsigned o_glist = ((unsigned)ecap + 2u) * 8u, o_any = o_glist + Bp * 4u;
  const unsigned dump = (unsigned)ecap, anydump = Bp;
  unsigned G;
  unsigned ovf0, n_places;  // the overflow area: the table's entries this scan does not use (pub_park_beyond_four)
  {
    const int tid = tid0;
    PubArgsPtr R = pub_args_now(rp);
    unsigned* glist = reinterpret_cast<unsigned*>(smem + o_glist);
    const unsigned* gb = R->glist;
    G = gb[B];
    const unsigned E = R->stats[0];
    ovf0 = (E + 1u) & ~1u;  // (an even entry: 16 bytes a place)
    n_places = (unsigned)ecap > ovf0 ? ((unsigned)ecap - ovf0) / 2u : 0u;
    if (n_places > 0xFFFEu) n_places = 0xFFFEu;
    for (int i = tid; i < B; i += kPubThreads) glist[i] = (unsigned)i < G ? gb[i] : 0u;
    for (unsigned i = (unsigned)tid; i < 2u * (Bp + 16u) / 4u; i += kPubThreads) reinterpret_cast<unsigned*>(smem + o_any)[i] = 0u;
    if (tid < kPubBigPlaces) s_bperm[tid] = reinterpret_cast<const unsigned short*>(gb + B + 1)[2 * kPubOctets + tid];
    if (tid < kPubBigSlots) s_rb[tid] = gb[B + 1 + kPubTailWords + tid];
    for (int i = tid; i < kPubUnmWords; i += kPubThreads) s_ubits[i] = 0u;
    if (tid == 0) {
      wg_flag[0] = 0;
      wg_flag[1] = 0;
      s_novf[0] = 0u;
      s_novf[1] = 0u;
    }
  }
  __syncthreads();

    // the rows of the pair at landmark lb_ of this particle's source slot
#define PK_BIG_ROWS(SA, SB, lb_, src_)                                                                \
  {                                                                                                   \
    PubArgsPtr R2 = pub_args_now(rp);                                                                 \
    const SlotSource ss_ = pub_slot_source(R2);                                                       \
    const unsigned char* sslot_ = ss_.at(src_);                                                       \
    const double* sf_ = reinterpret_cast<const double*>(sslot_);                                      \
    const int* sc_ = reinterpret_cast<const int*>(sslot_ + R2->count_off);                            \
    PK_BIG_LOAD(SA, SB, mx, F_MX, lb_)                                                                \
    PK_BIG_LOAD(SA, SB, my, F_MY, lb_)                                                                \
    PK_BIG_LOAD(SA, SB, mr, F_MR, lb_)                                                                \
    PK_BIG_LOAD(SA, SB, mg, F_MG, lb_)                                                                \
    PK_BIG_LOAD(SA, SB, mb, F_MB, lb_)                                                                \
    asm volatile("" ::: "memory");                                                                    \
    PK_BIG_LOAD(SA, SB, pxx, F_PXX, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, pxy, F_PXY, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, pyy, F_PYY, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, crr, F_CRR, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, crg, F_CRG, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, crb, F_CRB, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, cgg, F_CGG, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, cgb, F_CGB, lb_)                                                              \
    PK_BIG_LOAD(SA, SB, cbb, F_CBB, lb_)                                                              \
    const Int2 c_ = *reinterpret_cast<const Int2*>(sc_ + (lb_));                                      \
    SA.count = c_.x;                                                                                  \
    SB.count = c_.y;                                                                                  \
    asm volatile("" ::: "memory");                                                                    \
  }
  // (plain loads: non-temporal ones for pass 2's -- last -- read of the rows +8 %: that read does come from cache,
  // profiles/r04/ab_big_nontemporal_loads_pass2.log)
#define PK_BIG_LOAD(SA, SB, field, F, lb_)                                                            \
  {                                                                                                   \
    const Double2 v_ = *reinterpret_cast<const Double2*>(sf_ + (size_t)F * Lp + (lb_));              \
    SA.field = v_.x;                                                                                  \
    SB.field = v_.y;                                                                                  \
  }
  int64_t prev = -1;
  int cur = 0;
#ifdef PK_STAMPS
  // (diagnostic build: 0 pass 1 waits for records and rows | 1 gates | 2 verdicts | 3 next rows asked for | 4 barrier A | 5 settling, B |
  //  6 take, C | 7 pass 2 waits for rows | 8 updates | 9 particles | 10 stores, next rows asked for | 11 particle)
  unsigned long long pst[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PK_BIG_WAIT_ALL asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
#define PK_BIG_WAIT_ALL
#endif
  int32_t nsrc;  // the next particle's source slot, asked for a whole particle ahead (as in k_step_pub)
  {
    PubArgsPtr R = pub_args_now(rp);
    const int64_t p0 = PK_BIG_FIRST(R), pl = PK_BIG_LIMIT(R);
    nsrc = regs_source_pub(R->src, p0 < pl ? p0 : pl - 1);
  }
  // The rows of a pair are asked for as soon as the pair before it is through (into the registers it has just let go):
  // pair q + 1 behind pair q's verdicts in pass 1, pass 2's first pair behind the last verdicts (its rows fly during the
  // barriers and the settling), pair q + 1 behind pair q's stores in pass 2, and the NEXT particle's first pair behind the
  // last stores.
  Landmark<double> SA, SB;
  {
    const int lb0 = min(PK_BIG_L0(0, tid0), Lp - 2);
    PK_BIG_ROWS(SA, SB, lb0, nsrc)
  }
  for (int64_t p = PK_BIG_FIRST(pub_args_now(rp));; p += PK_BIG_STRIDE(), cur ^= 1) {
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int32_t csrc = nsrc;
    double* pub = reinterpret_cast<double*>(smem);
    const unsigned* glist = reinterpret_cast<const unsigned*>(smem + o_glist);
    unsigned char* anyc = smem + o_any + (unsigned)cur * (Bp + 16u);
    PubSlots Q[2 * NCH];
    double pse[2 * NCH];
#pragma unroll
    for (int i = 0; i < 2 * NCH; ++i) {
      Q[i] = kPubNoSlots;
      pse[i] = 0.0;
    }
    bool done;
    {
      PubArgsPtr R = pub_args_now(rp);
      done = p >= PK_BIG_LIMIT(R);
    }
    PK_STAMP(b0)
    // ---- pass 1: gates and verdicts, pair by pair
    // (ONE copy of the pair's code in a loop that is not unrolled -- written out per pair the kernel was 143 KB of
    // instructions, more than twice the instruction cache two CUs share -- with the carried words ROTATING through the
    // register arrays: a pair's results enter at the front, after NCH turns the LAST pair stands in front, where pass 2 begins)
    if (!done) {
#pragma unroll 1
      for (int q = 0; q < NCH; ++q) {
        PubSlots qa = kPubNoSlots, qb = kPubNoSlots;
        double pa = 0.0, pb = 0.0;
        if (2 * kPubThreads * q < Lp) {  // workgroup-uniform
          const int l0 = PK_BIG_L0(q, tid);
          PubArgsPtr R = pub_args_now(rp);
          PK_STAMP(c0)
          const double sx = pose_scalar(R->x, p), sy = pose_scalar(R->y, p), sh = pose_scalar(R->h, p);
#ifdef PK_DIAG_TAIL_LISTS
          const int lc = min(l0, Lp - 2);
#else
          const int lc = min(l0, Lp);  // (lanes beyond the map: the spare records, empty lists -- see k_step_pub)
#endif
          const uint4* cr = R->cand + 3 * (size_t)lc;
          const uint4* er = R->erec + 2 * (size_t)lc;
          PubGateIn gi[2];
          gi[0].ref = cr[0];
          gi[0].cw[0] = cr[1];
          gi[1].ref = cr[3];
          gi[1].cw[0] = cr[4];
          gi[0].ew[0] = er[0];
          gi[1].ew[0] = er[2];
          gi[0].cw[1] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
          gi[1].cw[1] = gi[0].cw[1];
          gi[0].ew[1] = gi[0].cw[1];
          gi[1].ew[1] = gi[0].cw[1];
          // (some landmark lists more than eight candidates: the second list word is read at all -- k_cand_entries' figure of the scan,
          // read here with the turn's other scalars: held across the particle loop it was one scalar register too many)
          if (R->stats[3] > (unsigned)kCandSlots) {  // kernel-uniform: once the lists are pruned, hardly ever (round 6: a third of the records' cache lines)
            gi[0].cw[1] = cr[2];
            gi[1].cw[1] = cr[5];
            gi[0].ew[1] = er[1];
            gi[1].ew[1] = er[3];
          }
          const uint4* frow = R->far;
          const bool far_hdr_on = frow != nullptr;
          uint4 fh0 = make_uint4(0u, 0u, 0u, 0u), fh1 = fh0;
          if (far_hdr_on) {
            fh0 = frow[3 * (size_t)lc];
            fh1 = frow[3 * (size_t)lc + 3];
          }
          asm volatile("" ::: "memory");
          // (this chunk's covariance rows asked for HERE, behind its candidate records, instead of with its means: 8.33 against
          // 8.08 ms -- the keys follow the gates too closely here; profiles/r04/ab_big_late_cov_rows.log)
          if (q == 0) {  // the next particle's source slot (as in k_step_pub)
            PubArgsPtr R4 = pub_args_now(rp);
            const int64_t pn = p + PK_BIG_STRIDE(), pl = PK_BIG_LIMIT(R4);
            nsrc = regs_source_pub(R4->src, pn < pl ? pn : pl - 1);
            asm volatile("" : "+s"(nsrc));
          }
          PK_BIG_WAIT_ALL
          PK_STAMP(c1)
          PK_PSTAMP(0, c0, c1)
          gi[0].mx = SA.mx;
          gi[0].my = SA.my;
          gi[0].mr = SA.mr;
          gi[0].mg = SA.mg;
          gi[0].mb = SA.mb;
          gi[0].has = l0 < L;
          gi[1].mx = SB.mx;
          gi[1].my = SB.my;
          gi[1].mr = SB.mr;
          gi[1].mg = SB.mg;
          gi[1].mb = SB.mb;
          gi[1].has = l0 + 1 < L;
          pub_far_bound(SA, gi[0].fk, gi[0].fi);
          pub_far_bound(SB, gi[1].fk, gi[1].fi);
          bool viol[2] = {false, false};
          if (far_hdr_on) {  // (uniform) do the scan's pruned lists hold for these two landmarks?
            viol[0] = gi[0].has && !(gi[0].fi >= (double)__uint_as_float(fh0.y) && gi[0].fk >= (double)__uint_as_float(fh0.x));
            viol[1] = gi[1].has && !(gi[1].fi >= (double)__uint_as_float(fh1.y) && gi[1].fk >= (double)__uint_as_float(fh1.x));
          }
          double pp[2] = {0.0, 0.0};
          const Landmark<double>* const l2[2] = {&SA, &SB};
          // Eight gate slots of which the positive ones -- at most four -- are kept.  (Four gate slots + the refill turn of
          // k_step_pub: 23.4 against 8.37 ms per step at 20 000 x 5 000 -- among 5 000 random colours a landmark with five to seven
          // gate-passing blobs is in nearly every WAVE's 128; profiles/r04/ab_big_four_slots_refill.log.)
          PubSlotsT<kPubBigGateSlots> qq[2];
          // the gates look at a candidate's float copy first (one 16-byte gather instead of two of the 48-byte record: 8.11 -> 7.75 ms,
          // ab_big_gate_float_table.log) and give look-alikes beyond the underflow edge no slot (-> 7.29 ms, ab_big_far_in_gates.log);
          // the verdicts take the key's constant term and the colour bound from them
          // (round 6) the two landmarks' primary blobs -- the fronts of their lists -- come from the table in landmark order: the float
          // records in the gates' first round, the exact ones where the verdicts want them
          pub_gatesN<2, 2, kPubBigGateSlots, false, true, true>(qq, pp, gi, R->exact, pub, dump, &wg_flag[cur], sx, sy, sh, R->gate4,
                                                                reinterpret_cast<const float4*>(R->prim), lc);
          PK_STAMP(c2)
          PK_PSTAMP(1, c1, c2)
          {
            const double kb_[2] = {gi[0].fk, gi[1].fk}, it_[2] = {gi[0].fi, gi[1].fi};
            {
              PubArgsPtr R8 = pub_args_now(rp);
              const uint4* fr8 = R8->far;
              pub_far_recheck<2, 2>(viol, l2, pp, kb_, it_, [&]() { return fr8 ? fr8 + 3 * (size_t)lc : (const uint4*)nullptr; }, R8->exact, sh, &wg_flag[cur]);
            }
            {
              PubArgsPtr R9 = pub_args_now(rp);
              PubPrim prim;
              prim.tab = R9->prim;
              prim.Lpp = (size_t)R9->Lp + kCandSpare;
              prim.lc = lc;
              pub_keysN<2, kPubBigGateSlots, true, false, 1, PubNoChk, true>(qq, l2, pp, R9->exact, pub, dump, anyc, anydump, &wg_flag[cur], sx, sy, kb_, it_,
                                                                             PubNoChk(), &prim);
            }
          }
          qa = pub_keep_positive(qq[0], nullptr);
          qb = pub_keep_positive(qq[1], nullptr);
          if (__ballot(__popc(qq[0].st & 0x11111111u) > kPubSlots || __popc(qq[1].st & 0x11111111u) > kPubSlots) != 0ull) {  // wave-uniform, rare
            uint4* ovf = reinterpret_cast<uint4*>(smem) + ovf0 / 2u;
            pub_park_beyond_four(qa, qq[0], ovf, n_places, &s_novf[cur], &wg_flag[cur]);
            pub_park_beyond_four(qb, qq[1], ovf, n_places, &s_novf[cur], &wg_flag[cur]);
          }
#if defined(PK_STAMPS) && defined(PK_DIAG_BIG_CERTAIN)
          {  // (diagnostic: how many wave.pairs hold only landmarks whose gate-passing blobs nobody else lists -- DESIGN.md section 10.2)
            bool cert = true;
#pragma unroll
            for (int s_ = 0; s_ < kPubSlots; ++s_) {
              if (((qa.st >> (4 * s_)) & 1u) && (qa.s[s_] >> 16) != 0xFFFFu) cert = false;
              if (((qb.st >> (4 * s_)) & 1u) && (qb.s[s_] >> 16) != 0xFFFFu) cert = false;
            }
            const unsigned long long bal = __ballot(cert);
            if ((tid & 63) == 0) {
              atomicAdd(&pk_pstamp_acc[12], bal == ~0ull ? 1ull : 0ull);
              atomicAdd(&pk_pstamp_acc[13], 1ull);
              atomicAdd(&pk_pstamp_acc[14], (unsigned long long)__popcll(bal));
            }
          }
#endif
          PK_STAMP(c3)
          PK_PSTAMP(2, c2, c3)
          pa = pp[0];
          pb = pp[1];
          // the next pair of this pass; the LAST pair's rows stay where they are: pass 2 starts with them (round 5: a fifth of the
          // second read at five pairs, a third at three, never asked for)
          // (six pairs: the registers do not stretch to it -- three of them spilled; pass 2 front to back from rows asked for again)
          if (kBack) {
            if (q + 1 < NCH && 2 * kPubThreads * (q + 1) < Lp) {  // workgroup-uniform
              const int ln = min(PK_BIG_L0(q + 1, tid), Lp - 2);
              PK_BIG_ROWS(SA, SB, ln, csrc)
            }
          } else {
            const bool more = q + 1 < NCH && 2 * kPubThreads * (q + 1) < Lp;  // workgroup-uniform
            const int ln = min(PK_BIG_L0(more ? q + 1 : 0, tid), Lp - 2);
            PK_BIG_ROWS(SA, SB, ln, csrc)
          }
#if defined(PK_STAMPS)
          PK_STAMP(c4)
          PK_PSTAMP(3, c3, c4)
#endif
        }
        if (kBack) {
#pragma unroll
          for (int i = 2 * NCH - 1; i >= 2; --i) {  // (a pair's results enter at the FRONT: pass 2 walks the pairs back to front)
            Q[i] = Q[i - 2];
            pse[i] = pse[i - 2];
          }
          Q[0] = qa;
          Q[1] = qb;
          pse[0] = pa;
          pse[1] = pb;
        } else {
#pragma unroll
          for (int i = 0; i + 2 < 2 * NCH; ++i) {
            Q[i] = Q[i + 2];
            pse[i] = pse[i + 2];
          }
          Q[2 * NCH - 2] = qa;
          Q[2 * NCH - 1] = qb;
          pse[2 * NCH - 2] = pa;
          pse[2 * NCH - 1] = pb;
        }
      }
    }
    PK_STAMP(b1)
    lds_barrier();  // A: every verdict of this particle is in the table
    PK_STAMP(b2)
    PK_PSTAMP(4, b1, b2)
    if (prev >= 0 && tid == 0) {  // the previous particle's log-weight (its partial sums were written before A)
      PubArgsPtr R = pub_args_now(rp);
      double tot = red[cur ^ 1][0];
#pragma unroll
      for (int i = 1; i < kPubWaves; ++i) tot += red[cur ^ 1][i];
      double* logw = R->logw;
      const double w = (R->reset ? 0.0 : logw[prev]) + tot;
      logw[prev] = w;
      unsigned long long* gk = R->gmax_key;
      if (gk) atomicMax(gk + (prev & (kGmaxKeys - 1)), double_to_key(w));
      R->src[prev] = (int32_t)prev;
    }
    if (done) break;
    prev = -1;
    double acc;
    {
      int nun = 0;
      for (unsigned w = (unsigned)tid; w < Bp / 4u; w += kPubThreads) {
        const unsigned v = reinterpret_cast<const unsigned*>(anyc)[w];
#pragma unroll
        for (int b = 0; b < 4; ++b) nun += ((int)(4 * w + b) < B && ((v >> (8 * b)) & 0xFFu) == 0u) ? 1 : 0;
      }
      acc = (double)nun * Consts<double>::log_no_match;  // unseen features: weight *= 0.1 each (:94-95)
      unsigned* anyn = reinterpret_cast<unsigned*>(smem + o_any + (unsigned)(cur ^ 1) * (Bp + 16u));
      for (unsigned w = (unsigned)tid; w < Bp / 4u; w += kPubThreads) anyn[w] = 0u;
      if (tid == 0) {  // (the other parity's: its particle's markers were read before its barrier C, the next one's pass 1 starts behind this one's C)
        wg_flag[cur ^ 1] = 0;
        s_novf[cur ^ 1] = 0u;
      }
    }
    {
      PubArgsPtr Ru = pub_args_now(rp);
      if (Ru->unm != nullptr) pub_note_unmatched<kPubThreads>(tid, anyc, Ru->order, B, Bp, s_ubits);  // kernel-uniform: growing maps only
    }
    pub_settle_blobs<kPubThreads, kPubBigSlots>(tid, glist, G, pub, dump, &wg_flag[cur], s_rb);
    lds_barrier();  // B: every winner is marked, every flag is set
    PK_STAMP(b3)
    PK_PSTAMP(5, b2, b3)
    {
      PubArgsPtr Ru = pub_args_now(rp);
      if (Ru->unm != nullptr) pub_store_unmatched<kPubThreads>(tid, s_ubits, Ru->unm + (size_t)p * Ru->unm_words, Ru->unm_words);
    }
#pragma unroll
    for (int i = 0; i < 2 * NCH; ++i) pub_take(Q[i], pub, dump);
    if (s_novf[cur] != 0u) {  // workgroup-uniform (written before barrier A; the other parity's is reset between A and B): some landmark parked blobs
#pragma unroll
      for (int i = 0; i < 2 * NCH; ++i) pub_take_parked(Q[i], reinterpret_cast<const uint4*>(smem) + ovf0 / 2u, pub, dump, &wg_flag[cur]);
    }
    lds_barrier();  // C: every marker has been read -- the table is the next particle's
    PK_STAMP(b4)
    PK_PSTAMP(6, b3, b4)
    if (wg_flag[cur]) {  // workgroup-uniform: nothing has been written; the fall-back kernels take the particle
      if (tid == 0) {
        PubArgsPtr R = pub_args_now(rp);
        R->pflag_out[p] = 1;
        atomicAdd(R->n_flagged, 1u);
      }
      {  // (the registers hold this particle's first pair: the next particle's instead)
        const int lb0 = min(PK_BIG_L0(0, tid), Lp - 2);
        PK_BIG_ROWS(SA, SB, lb0, nsrc)
      }
      continue;
    }
    if (tid == 0) pub_args_now(rp)->pflag_out[p] = 0;
    // ---- pass 2: rows in again, updates in scan order, rows out
    // (Measured and dropped, round 4: the record of a landmark's blob asked for a pair AHEAD of its update, +0.9 % --
    // ab_big_apply_records_a_pair_ahead.log; wave priorities in pass 2 -- ab_big_wave_priorities.log; plain stores, +8 % --
    // ab_big_plain_stores.log.)
#define PK_BIG_STORE(field, F)                                                             \
  {                                                                                        \
    const Double2 v_ = {SA.field, SB.field};                                               \
    __builtin_nontemporal_store(v_, reinterpret_cast<Double2*>(df + (size_t)F * Lp + l0)); \
  }
    // (back to front: the pair pass 1 ended on is still in the registers)
    double nprod = 1.0;  // (the product of the norms of this lane's updates: pub_fold_norms)
#pragma unroll 1
    for (int qr = 0; qr < NCH; ++qr) {
      const int q = kBack ? NCH - 1 - qr : qr;
      if (2 * kPubThreads * q < Lp) {  // workgroup-uniform
        const int l0 = PK_BIG_L0(q, tid);
        PubArgsPtr R = pub_args_now(rp);
        PK_STAMP(d0)
        PK_BIG_WAIT_ALL
        PK_STAMP(d1)
        PK_PSTAMP(7, d0, d1)
        const Noise<double> qt = pub_noise(R);
        const double sx = pose_scalar(R->x, p), sy = pose_scalar(R->y, p);
        const unsigned char* immutable = R->immutable;
        // (the scan-order table in global memory: see pub_big_fixed_lds_bytes)
        // (the blob a landmark applies is nearly always its primary one: its exact record from the table in landmark order)
        const int lc2 = min(l0, Lp);
        const size_t Lpp = (size_t)Lp + kCandSpare;
        const uint2 tt = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned*>(R->prim + 4 * Lpp) + lc2);
        acc += pub_apply_loop<true>(Q[0], R->exact, R->order, qt, SA, immutable[min(l0, L - 1)] != 0, sx, sy, pse[0],
                                    reinterpret_cast<const char*>(R->prim + Lpp), Lpp * 16, lc2, tt.x, PK_PROD_PTR(nprod));
        {
          PubArgsPtr R8 = pub_args_now(rp);
          acc += pub_apply_loop<true>(Q[1], R8->exact, R8->order, qt, SB, immutable[min(l0 + 1, L - 1)] != 0, sx, sy, pse[1],
                                      reinterpret_cast<const char*>(R8->prim + Lpp), Lpp * 16, lc2 + 1, tt.y, PK_PROD_PTR(nprod));
        }
        PK_STAMP(d2)
        PK_PSTAMP(8, d1, d2)
        if (l0 < Lp) {
          PubArgsPtr R3 = pub_args_now(rp);
          unsigned char* dslot = R3->map_dst + (size_t)p * R3->ss.slot_bytes;
          double* df = reinterpret_cast<double*>(dslot);
          int* dc = reinterpret_cast<int*>(dslot + R3->count_off);
          PK_BIG_STORE(mx, F_MX)
          PK_BIG_STORE(my, F_MY)
          PK_BIG_STORE(mr, F_MR)
          PK_BIG_STORE(mg, F_MG)
          PK_BIG_STORE(mb, F_MB)
          PK_BIG_STORE(pxx, F_PXX)
          PK_BIG_STORE(pxy, F_PXY)
          PK_BIG_STORE(pyy, F_PYY)
          PK_BIG_STORE(crr, F_CRR)
          PK_BIG_STORE(crg, F_CRG)
          PK_BIG_STORE(crb, F_CRB)
          PK_BIG_STORE(cgg, F_CGG)
          PK_BIG_STORE(cgb, F_CGB)
          PK_BIG_STORE(cbb, F_CBB)
          const Int2 c2_ = {SA.count, SB.count};
          __builtin_nontemporal_store(c2_, reinterpret_cast<Int2*>(dc + l0));
        }
        {  // the pair before it (front to back: behind it), or the next particle's first one
          const bool more = kBack ? q > 0 : (q + 1 < NCH && 2 * kPubThreads * (q + 1) < Lp);  // workgroup-uniform
          const int ln = min(PK_BIG_L0(more ? (kBack ? q - 1 : q + 1) : 0, tid), Lp - 2);
          const int32_t sn = more ? csrc : nsrc;
          PK_BIG_ROWS(SA, SB, ln, sn)
        }
        PK_STAMP(d3)
        PK_PSTAMP(10, d2, d3)
      }
#pragma unroll
      for (int i = 0; i + 2 < 2 * NCH; ++i) {  // the words of the pair before it to the front
        Q[i] = Q[i + 2];
        pse[i] = pse[i + 2];
      }
    }
#undef PK_BIG_STORE
#undef PK_BIG_ROWS
#undef PK_BIG_LOAD
    pub_fold_norms(acc, nprod);
    {
      const double ws = wave_sum(acc);  // the sum over the workgroup is finished behind the next barrier A
      if ((tid & (kWave - 1)) == 0) red[cur][tid / kWave] = ws;
      prev = p;
    }
#ifdef PK_STAMPS
    {
      PK_STAMP(b5)
      PK_PSTAMP(11, b0, b5)
      pst[9] += 1ull;
    }
#endif
  }
#ifdef PK_STAMPS
  if ((tid0 & 63) == 0)
    for (int k = 0; k < 12; ++k) atomicAdd(&pk_pstamp_wave[tid0 >> 6][k], pst[k]);
#endif
#undef PK_BIG_WAIT_ALL
}

// What the three launchers of this file hand their kernel alike; `skip`, `ecap`, `stats` and the two-pass members are each one's own
static PubArgs pub_args(const DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt, const ObserveExtras& ex,
                        const PubTables& pub, const ParticleRange& range) {
  PubArgs a{};
  fill_state(a, d);
  fill_scan(a, scan, ex, qt);
  a.cand = pub.cand.rec;
  a.far = pub.cand.far;
  a.erec = pub.erec;
  a.glist = pub.glist;
  a.unm = ex.unm;
  a.unm_words = ex.unm_words;
  a.pflag_out = fh.pflag;
  a.n_flagged = fh.n_flagged;
  a.P = range.end(d.P);
  a.p_begin = range.p0;
  return a;
}

void launch_step_pub_big(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                         const ObserveExtras& ex, const PubTables& pub, const ParticleRange& range) {
  // persistent grid, one workgroup per CU
  const int64_t grid_n = persistent_grid(device_cu_count(), 1, range, d.P);
  if (grid_n == 0) return;
  static bool attr_set[kMaxDevices] = {false};
  allow_dynamic_lds(attr_set, kMaxDynLds, k_step_pub_big<3>, k_step_pub_big<5>, k_step_pub_big<6>);
  PubArgs a = pub_args(d, scan, fh, qt, ex, pub, range);
  a.skip = pub.skip_big;
  a.gate4 = pub.gate4;
  a.prim = pub.prim;
  a.stats = pub.stats;
  a.ecap = pub.ecap;
  const size_t lds = step_pub_big_lds_bytes(scan.B, pub.ecap);
  const int nch = (d.lay.Lp + 2 * kPubThreads - 1) / (2 * kPubThreads);
  if (nch <= 3)
    hipLaunchKernelGGL(k_step_pub_big<3>, dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
  else if (nch <= 5)
    hipLaunchKernelGGL(k_step_pub_big<5>, dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
  else
    hipLaunchKernelGGL(k_step_pub_big<6>, dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
}

void launch_step_pub(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                     const ObserveExtras& ex, const PubTables& pub, const ParticleRange& range) {
  // persistent grid: one workgroup per CU (512 lanes x 256 VGPRs), three of the 256-lane instance (143 VGPRs; LDS permitting)
  const bool small = d.lay.Lp <= 2 * kPubSmallThreads;
  const size_t lds = step_pub_lds_bytes(scan.B, pub.ecap, small);
  int per_cu = 1;
  if (small) per_cu = (int)std::min<size_t>(3, std::max<size_t>(1, (160 * 1024 - 1024) / (lds + 256)));
  const int64_t grid_n = persistent_grid(device_cu_count(), per_cu, range, d.P);
  if (grid_n == 0) return;
  static bool attr_set[kMaxDevices] = {false};
  allow_dynamic_lds(attr_set, kMaxDynLds, k_step_pub<1, kPubSmallThreads>, k_step_pub<1, kPubThreads>, k_step_pub<2, kPubThreads>,
                    k_step_pub<1, kPubThreads, true>, k_step_pub<2, kPubThreads, true>);
  PubArgs a = pub_args(d, scan, fh, qt, ex, pub, range);
  a.skip = pub.skip_pub;
  a.stats = ex.lean_stats;
  a.ecap = pub.ecap;
  const bool tab = ex.ctab != nullptr && !small;
  a.ctab = tab ? ex.ctab : nullptr;
  a.ctab_max = ex.ctab_max;
  a.ctab_depth = ex.ctab_depth;
  a.lean = ex.lean;
  if (small)
    hipLaunchKernelGGL((k_step_pub<1, kPubSmallThreads>), dim3((unsigned)grid_n), dim3(kPubSmallThreads), lds, s, a);
  else if (d.lay.Lp <= 2 * kPubThreads) {
    if (tab)
      hipLaunchKernelGGL((k_step_pub<1, kPubThreads, true>), dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
    else
      hipLaunchKernelGGL((k_step_pub<1, kPubThreads>), dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
  } else {
    if (tab)
      hipLaunchKernelGGL((k_step_pub<2, kPubThreads, true>), dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
    else
      hipLaunchKernelGGL((k_step_pub<2, kPubThreads>), dim3((unsigned)grid_n), dim3(kPubThreads), lds, s, a);
  }
}

#include "pk_k_step_duo.inl"

}  // namespace pk
