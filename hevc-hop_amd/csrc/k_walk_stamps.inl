// k_walk_stamps.inl -- stage stamps of the candidate walks (included by k_cabac.hip in front of k_leaf_fused.inl; the stages and the table: include/hophip.h).
//
// HOP_WALK_STAMPS undefined (libhophip.so): the four macros below expand to nothing and this file adds no device code.
// HOP_WALK_STAMPS defined (libhophip_stamps.so, a diagnostic build): thread 0 of a workgroup keeps ONE timeline.  WS_BEGIN() at the kernel's entry takes the first stamp
// and opens HOP_WS_OTHER; WS(stage) takes a stamp, adds the cycles since the last one to the stage that was open and opens `stage`; WS_END(kernel, log2_cu, nxn) closes
// the open stage with the last stamp and adds the workgroup's sums to the device table g_ws_table with 64-bit atomics.  Only thread 0 touches the accumulators, so they
// need no barrier; they are a __shared__ object at file scope (as s_bin_table): leaf_serial and the other bodies that are functions of their own reach it by name with
// ds_* instructions, no pointer travels through their signatures.
// A stamp is one asm statement -- the clock read and the wait for it -- between two scheduling barriers (the compiler moves nothing across it).  It costs some tens of
// cycles and its wait drains the lane's LDS / scalar-memory counter, its bookkeeping is a handful of LDS operations: the build is slower than the product, and what its
// table says are SHARES of thread 0's timeline.  hop_walk_stamps_probe measures the cost so that it can be stated beside them.
// The leaf bodies are shared with the batch-step kernels (k_turd_fused*, k_rqt_*), which have no WS_BEGIN / WS_END: there the stamps of the leaf add into accumulators
// nobody reads (the index of the open stage is masked into the array, whatever the uninitialised LDS holds).
#ifndef HOP_WALK_STAMPS
#define WS_BEGIN()
#define WS(stage)
#define WS_IF(cond, stage)
#define WS_END(kernel, log2_cu, nxn)
#else
#define WS_SLOTS 16                                                   // HOP_WS_COUNT rounded up to a power of two (the mask above)
#define WS_ROW (2 * HOP_WS_COUNT + 4)                                 // cycles per stage, visits per stage, workgroups, cycles, realtime ticks, longest realtime span
static_assert(HOP_WS_COUNT <= WS_SLOTS, "WS_SLOTS");
__device__ unsigned long long g_ws_table[HOP_WSK_COUNT][4][2][WS_ROW];
__device__ unsigned long long g_ws_probe[4];
struct WsLds { unsigned long long cyc[WS_SLOTS], vis[WS_SLOTS], first, last, rt_first; int open; };
__shared__ WsLds s_ws;

__device__ static __forceinline__ unsigned long long ws_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
__device__ static __forceinline__ unsigned long long ws_realtime() {   // the constant 100 MHz counter
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
__device__ static __forceinline__ void ws_begin() {
  if (threadIdx.x != 0) return;
  for (int s = 0; s < WS_SLOTS; s++) { s_ws.cyc[s] = 0; s_ws.vis[s] = 0; }
  s_ws.open = HOP_WS_OTHER; s_ws.vis[HOP_WS_OTHER] = 1;
  s_ws.rt_first = ws_realtime();
  const unsigned long long t = ws_stamp();
  s_ws.first = t; s_ws.last = t;
}
__device__ static __forceinline__ void ws_mark(const int stage) {
  if (threadIdx.x != 0) return;
  const unsigned long long now = ws_stamp();
  s_ws.cyc[s_ws.open & (WS_SLOTS - 1)] += now - s_ws.last;
  s_ws.last = now; s_ws.open = stage; s_ws.vis[stage] += 1;
}
__device__ static __forceinline__ void ws_end(const int kernel, const int log2_cu, const int nxn) {
  if (threadIdx.x != 0) return;
  const unsigned long long now = ws_stamp();
  s_ws.cyc[s_ws.open & (WS_SLOTS - 1)] += now - s_ws.last;
  const unsigned long long rt = ws_realtime() - s_ws.rt_first;        // (taken outside the two cycle stamps: it spans them)
  if (kernel < 0 || kernel >= HOP_WSK_COUNT || log2_cu < 3 || log2_cu > 6) return;
  unsigned long long* row = g_ws_table[kernel][log2_cu - 3][nxn ? 1 : 0];
  for (int s = 0; s < HOP_WS_COUNT; s++) {
    const unsigned long long c = s_ws.cyc[s], v = s_ws.vis[s];
    if (c) atomicAdd(row + s, c);
    if (v) atomicAdd(row + HOP_WS_COUNT + s, v);
  }
  atomicAdd(row + 2 * HOP_WS_COUNT, 1ull);
  atomicAdd(row + 2 * HOP_WS_COUNT + 1, now - s_ws.first);
  atomicAdd(row + 2 * HOP_WS_COUNT + 2, rt);
  atomicMax(row + 2 * HOP_WS_COUNT + 3, rt);
}
#define WS_BEGIN() ws_begin()
#define WS(stage) ws_mark(stage)
#define WS_IF(cond, stage) do { if (cond) ws_mark(stage); } while (0)
#define WS_END(kernel, log2_cu, nxn) ws_end(kernel, log2_cu, nxn)

// the instrument on itself: one workgroup, thread 0
#define WS_PROBE_ROUNDS 4096
__global__ __launch_bounds__(256) void k_ws_probe() {
  WS_BEGIN();
  if (threadIdx.x != 0) return;
  unsigned long long best = ~0ull;
  const unsigned long long r0 = ws_realtime(), t0 = ws_stamp();
  for (int q = 0; q < WS_PROBE_ROUNDS; q++) {
    const unsigned long long a = ws_stamp(), b = ws_stamp();
    if (b - a < best) best = b - a;
  }
  const unsigned long long t1 = ws_stamp(), r1 = ws_realtime();
  WS(HOP_WS_OTHER);
  for (int q = 0; q < WS_PROBE_ROUNDS; q++) WS(HOP_WS_TAIL);             // every round charges one boundary's own cost to TAIL
  WS(HOP_WS_OTHER);
  g_ws_probe[0] = best; g_ws_probe[1] = s_ws.cyc[HOP_WS_TAIL] / WS_PROBE_ROUNDS; g_ws_probe[2] = t1 - t0; g_ws_probe[3] = r1 - r0;
}
#endif
