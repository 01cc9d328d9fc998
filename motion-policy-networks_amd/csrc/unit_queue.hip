// unit_queue.hip -- the pool of device-side unit queues that the persistent grouped-MLP kernels take their work from
// (sa_mlp.hip's packed kernel, sa_mlp_bf16.hip's persistent kernel; declared in common.h).
#include "common.h"

#include <mutex>
#include <unordered_map>

// Unit queues of the persistent kernels: 8 counters (one per XCD) per launch, in device memory that belongs to the
// library image (nothing is allocated).  ONE SLOT PER (device, stream): the launches of a stream are ordered (memset,
// kernel, memset, kernel, ...), so they can share a slot, and launches on different streams never alias -- two engines
// that share a model on two streams each get their own counters.  The slot is zeroed on the
// launch stream in front of the kernel (stream-ordered, hipGraph-capturable).  Limits, stated in include/mpinets_hip.h:
// 256 distinct (device, stream) handles per process get a slot; a later handle gets NONE (`*exhausted` = 1, nullptr):
// slots are never shared between streams -- two persistent kernels on one set of counters would each skip the units
// the other claimed and leave output rows unwritten -- so the fp32 launchers fall back to their one-unit-per-wave
// grids and the bf16x3 launcher reports an error.  A captured graph bakes its capture stream's slot in, so two graphs
// captured on the SAME stream must not be replayed concurrently on different streams.
__device__ unsigned int sa2_unit_queues[256 * 8];
unsigned int *mpx_unit_queue_for(hipStream_t stream, int *exhausted) {
  static std::mutex mu;
  static std::unordered_map<unsigned long long, int> slot_of;  // (device << 56) ^ stream handle -> slot
  static unsigned int *base[64];
  if (exhausted) *exhausted = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  unsigned int *q;
  {
    std::lock_guard<std::mutex> lock(mu);
    unsigned int *&b = base[dev & 63];
    if (!b) {
      void *p = nullptr;
      if (hipGetSymbolAddress(&p, HIP_SYMBOL(sa2_unit_queues)) != hipSuccess) return nullptr;
      b = static_cast<unsigned int *>(p);
    }
    const unsigned long long key = ((unsigned long long)(dev & 63) << 56) ^ (unsigned long long)(uintptr_t)stream;
    auto it = slot_of.find(key);
    if (it == slot_of.end()) {
      if (slot_of.size() >= (size_t)mpx_unit_queue_slots()) {
        if (exhausted) *exhausted = 1;
        return nullptr;
      }
      it = slot_of.emplace(key, (int)slot_of.size()).first;
    }
    q = b + 8 * it->second;
  }
  if (hipMemsetAsync(q, 0, 8 * sizeof(unsigned int), stream) != hipSuccess) return nullptr;
  return q;
}
// (verification hook: tests shrink the slot count to reach the exhausted path without creating 256 streams)
static std::atomic<int> unit_queue_slots{256};
int mpx_unit_queue_slots() { return unit_queue_slots.load(); }
void mpx_unit_queue_set_slots(int n) { unit_queue_slots.store(n < 0 ? 0 : n > 256 ? 256 : n); }
