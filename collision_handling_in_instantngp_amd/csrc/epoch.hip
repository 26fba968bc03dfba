// The epoch loop of the reference's grid_search_loop (functions.py:639-814) without a host in it: after every epoch one
// small launch takes the stop and save decisions from numbers that are on the device already — the per-batch losses, the
// image's two integer sums, the distinct-slot counts — and a predicated multi-tensor copy keeps the best state in a device
// snapshot instead of five torch.save files.  The host enqueues N epochs and polls one word now and then.
#include "gngf_common.h"

#include <math.h>

namespace gngf {

struct EpochState {         // mirrored by the host (train.py: EPOCH_STATE); 128 bytes
  int32_t take;             // this epoch's state is the new best (train_psnr >= best_psnr, functions.py:761)
  int32_t last;             // this epoch is the run's last (the reference's `break`, or epoch epochs - 1)
  int32_t finished;         // the last epoch has been recorded: further calls only clear take and last
  int32_t stop;             // early_stopper.early_stop
  int32_t reason;           // written with `finished`: 1 epochs reached, 2 the early stopper, 3 zero collisions
  int32_t cause;            // who set `stop` first: 0 nobody, 2 the early stopper, 3 the zero-collision rule
  int32_t zero_checks;      // len(check_last2_collisions)
  int32_t zero_all;         // all(check_last2_collisions) so far
  int64_t epoch;            // epochs recorded = index of the next one
  int64_t counter;          // early_stopper.counter
  int64_t best_sse;         // integer form of best_psnr (host: sse_limit0)
  int64_t best_epoch;       // -1: none yet
  int64_t last_epoch;       // -1: still running
  double best_loss;         // early_stopper.best_loss
  int64_t reserved[6];
};
static_assert(sizeof(EpochState) == 128, "host layout");

constexpr int kLogIntFixed = 6;      // eq, sse, counter, saved, stopper fired, zero-collision stop; then used (Kc, L)

// np.mean of nb float64 values, nb < 8: a sequential sum in order, then one division (numpy's pairwise sum adds
// blocks of fewer than 8 elements in a plain loop)
__device__ __forceinline__ double mean_in_order(const float* __restrict__ v, int nb, int stride) {
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += (double)v[(int64_t)b * stride];
  return s / (double)nb;
}

// One workgroup of one wave.  Lanes share the per-level means; lane 0 runs the state machine in plain double / int64.
__global__ void __launch_bounds__(64)
epoch_tail_kernel(EpochState* __restrict__ st, double* __restrict__ logf, int64_t* __restrict__ logi,
                  const float* __restrict__ loss, const float* __restrict__ mse, const float* __restrict__ kls,
                  const float* __restrict__ colls, int nb, int L, const int64_t* __restrict__ sums,
                  const int32_t* __restrict__ used, int Kc, int hash_source, const int64_t* __restrict__ nverts,
                  double tolerance, double min_delta, int should_reset, int64_t epochs) {
  const int finished = st->finished;
  const int64_t e = st->epoch;
  __syncthreads();                                        // every lane has read the state before lane 0 changes it
  if (finished || e >= epochs) {
    if (threadIdx.x == 0) { st->take = 0; st->last = 0; }
    return;
  }
  const int nf = 2 + 2 * L, ni = kLogIntFixed + Kc * L;
  double* rowf = logf + e * nf;
  int64_t* rowi = logi + e * ni;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int l = threadIdx.x; l < L; l += 64) {
    rowf[2 + l] = kls ? mean_in_order(kls + l, nb, L) : nan;
    rowf[2 + L + l] = colls ? mean_in_order(colls + l, nb, L) : nan;
  }
  for (int i = threadIdx.x; i < Kc * L; i += 64) rowi[kLogIntFixed + i] = (int64_t)used[i];
  if (threadIdx.x != 0) return;

  const double train_loss = mean_in_order(loss, nb, 1);
  rowf[0] = train_loss;
  rowf[1] = mean_in_order(mse, nb, 1);
  const int64_t eq = sums[0], sse = sums[1];
  int stop = st->stop, cause = st->cause;
  int64_t counter = st->counter;

  // functions.py:681-688: in each of the epochs 1..10, are the last two levels free of collisions?
  int zero_stop = 0;
  if (used && Kc > 0 && e != 0 && st->zero_checks < 10) {
    bool zero = true;
    for (int l = (L >= 2 ? L - 2 : 0); l < L; ++l) {
      if (hash_source) {
        zero = zero && (nverts[l] - (int64_t)used[l] == 0);
      } else {                                            // mean over k, clamped at 0, == 0  <=>  the integer sum <= 0
        int64_t s = 0;
        for (int k = 0; k < Kc; ++k) s += nverts[l] - (int64_t)used[k * L + l];
        zero = zero && (s <= 0);
      }
    }
    const int checks = st->zero_checks + 1;
    const int all = st->zero_all && zero;
    st->zero_checks = checks;
    st->zero_all = all;
    if (checks == 10 && all) {
      zero_stop = 1;
      stop = 1;
      if (cause == 0) cause = 3;
    }
  }

  // functions.py:761: train_psnr >= best_psnr, decided on the integers (the order of the float PSNRs)
  int take = 0;
  if (sse <= st->best_sse) {
    st->best_sse = sse;
    st->best_epoch = e;
    take = 1;
  }

  // functions.py:783-794: the break, before this epoch's loss reaches the stopper
  int last = 0, fired = 0, reason = 0;
  if (stop) {
    last = 1;
    reason = cause;
  } else {
    if (e != 0) {                                         // utils.py:186-205, branch by branch
      double best = st->best_loss;
      const double d = fabs(best - train_loss);
      if (d < min_delta && train_loss < best) {
        counter += 1;
      } else if (d > min_delta && train_loss > best) {
        counter += 1;
      } else if (!should_reset) {
        counter = counter <= 0 ? 0 : counter - 1;
      } else {
        counter = 0;
        best = train_loss;
      }
      st->best_loss = best;
      if ((double)counter >= tolerance) {
        fired = 1;
        stop = 1;
        if (cause == 0) cause = 2;
      }
    }
    if (e == epochs - 1) {
      last = 1;
      reason = 1;
    }
  }
  rowi[0] = eq;
  rowi[1] = sse;
  rowi[2] = counter;
  rowi[3] = take;
  rowi[4] = fired;
  rowi[5] = zero_stop;
  st->counter = counter;
  st->stop = stop;
  st->cause = cause;
  st->epoch = e + 1;
  st->take = take;
  st->last = last;
  if (last) {
    st->last_epoch = e;
    st->reason = reason;
    st->finished = 1;
  }
}

struct SnapshotRecord {     // mirrored by the host packer (train.py: DeviceSnapshot.pack_records); 32 bytes
  const void* src;
  void* dst;
  int64_t bytes;
  int64_t first_block;
};
static_assert(sizeof(SnapshotRecord) == 32, "host packer layout");

constexpr int kSnapThreads = 256;
constexpr int kSnapBlockBytes = kSnapThreads * 16 * 4;   // four 16-byte accesses per lane

// Workgroup `blk` copies bytes [off, off + kSnapBlockBytes) of the record it belongs to (bisection on first_block, as the
// Adam kernel finds its segment) — if *flag is non-zero.  The block size is a multiple of 16, so a block starts as
// aligned as its tensor does.
__global__ void __launch_bounds__(kSnapThreads)
snapshot_if_kernel(const SnapshotRecord* __restrict__ recs, int nrec, const int32_t* __restrict__ flag) {
  if (*flag == 0) return;
  __shared__ int s_rec;
  const int64_t blk = blockIdx.x;
  if (threadIdx.x == 0) {
    int lo = 0, hi = nrec - 1;                            // last record with first_block <= blk
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (recs[mid].first_block <= blk) lo = mid; else hi = mid - 1;
    }
    s_rec = lo;
  }
  __syncthreads();
  const SnapshotRecord r = recs[s_rec];
  const int64_t off = (blk - r.first_block) * kSnapBlockBytes;
  if (off >= r.bytes) return;
  const int64_t len = r.bytes - off < kSnapBlockBytes ? r.bytes - off : kSnapBlockBytes;
  const unsigned char* s = static_cast<const unsigned char*>(r.src) + off;
  unsigned char* d = static_cast<unsigned char*>(r.dst) + off;
  const uintptr_t both = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d);
  int64_t done = 0;                                       // bytes [0, done) are covered by the wide loop
  if ((both & 15) == 0) {
    const int64_t n16 = len >> 4;
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* d4 = reinterpret_cast<uint4*>(d);
    for (int64_t i = threadIdx.x; i < n16; i += kSnapThreads) d4[i] = s4[i];
    done = n16 << 4;
  } else if ((both & 3) == 0) {
    const int64_t n4 = len >> 2;
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(s);
    uint32_t* d1 = reinterpret_cast<uint32_t*>(d);
    for (int64_t i = threadIdx.x; i < n4; i += kSnapThreads) d1[i] = s1[i];
    done = n4 << 2;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += kSnapThreads) d[i] = s[i];
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_epoch_state_bytes(void) { return (int)sizeof(EpochState); }
extern "C" int gngf_epoch_log_int_columns(int Kc, int L) { return kLogIntFixed + Kc * L; }

extern "C" int gngf_epoch_tail(void* state, double* logf, int64_t* logi, const float* loss, const float* mse, const float* kls,
                               const float* colls, int nb, int L, const int64_t* sums, const int32_t* used, int Kc, int hash_source,
                               const int64_t* nverts, double tolerance, double min_delta, int should_reset, int64_t epochs,
                               void* stream) {
  GNGF_CHECK_ARG(state && logf && logi && loss && mse && sums && nb >= 1 && L >= 1 && epochs >= 1);
  GNGF_CHECK_ARG((used != nullptr) == (Kc > 0) && Kc >= 0 && (!used || nverts) && (!hash_source || Kc <= 1));
  GNGF_CHECK_ARG(((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(logf) | reinterpret_cast<uintptr_t>(logi) |
                   reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(nverts)) & 7) == 0);
  epoch_tail_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(static_cast<EpochState*>(state), logf, logi, loss, mse, kls, colls,
                                                                 nb, L, sums, used, Kc, hash_source, nverts, tolerance, min_delta,
                                                                 should_reset, epochs);
  GNGF_RETURN_LAUNCH();
}

extern "C" int gngf_snapshot_block_bytes(void) { return kSnapBlockBytes; }

extern "C" int gngf_snapshot_if(const void* records, int nrec, int64_t total_blocks, const int32_t* flag, void* stream) {
  GNGF_CHECK_ARG(records && flag && nrec >= 1 && total_blocks >= 1 && total_blocks <= 0x7fffffffll);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(records) & 7) == 0 && (reinterpret_cast<uintptr_t>(flag) & 3) == 0);
  snapshot_if_kernel<<<dim3((unsigned)total_blocks), dim3(kSnapThreads), 0, as_stream(stream)>>>(
      static_cast<const SnapshotRecord*>(records), nrec, flag);
  GNGF_RETURN_LAUNCH();
}
