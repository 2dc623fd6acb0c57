// Stand-alone check of the filter's memory registry (parakeet_slam_amd/csrc/pk_devmem.hpp) over malloc / free: no GPU, no HIP.
// tests/test_devmem_host.py builds it with -fsanitize=address,undefined and runs it; it prints "devmem ok" and exits 0, or
// names the first check that failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../parakeet_slam_amd/csrc/pk_devmem.hpp"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

namespace {

constexpr int kNoMem = -5;

// what the stand-ins have handed out and not got back; shared by every copy of the policy
struct Heap {
  std::map<void*, size_t> device, host;
  long calls = 0;     // allocations asked for, failed ones included
  long fail_at = -1;  // the allocation with this number (counted from 0) fails
  size_t sum(const std::map<void*, size_t>& m) const {
    size_t s = 0;
    for (const auto& kv : m) s += kv.second;
    return s;
  }
};

struct FakeRaw {
  Heap* heap = nullptr;
  int take(std::map<void*, size_t>& m, void** p, size_t bytes) {
    if (heap->calls++ == heap->fail_at) return kNoMem;
    *p = std::malloc(bytes ? bytes : 1);
    CHECK(*p);
    std::memset(*p, 0xA5, bytes);  // (the whole block is the caller's: the sanitizer sees a short one)
    m[*p] = bytes;
    return 0;
  }
  void give(std::map<void*, size_t>& m, void* p) {
    CHECK(m.count(p) == 1);  // freed once, and through the call that matches its kind
    m.erase(p);
    std::free(p);
  }
  int device_alloc(void** p, size_t bytes) { return take(heap->device, p, bytes); }
  void device_free(void* p) { give(heap->device, p); }
  int host_alloc(void** p, size_t bytes, unsigned) { return take(heap->host, p, bytes); }
  void host_free(void* p) { give(heap->host, p); }
};

using Mem = pk::DevMem<FakeRaw>;

void check_totals(const Mem& mem, const Heap& heap) {
  CHECK(mem.device_bytes() == heap.sum(heap.device));
  CHECK(mem.host_bytes() == heap.sum(heap.host));
  CHECK(mem.live_blocks() == heap.device.size() + heap.host.size());
}

int g_quiesced = 0;
int quiesce() {
  ++g_quiesced;
  return 0;
}

void test_alloc_release() {
  Heap heap;
  Mem mem(FakeRaw{&heap});
  double* a = nullptr;
  int32_t* b = nullptr;
  unsigned* h = nullptr;
  CHECK(mem.alloc(&a, 10) == 0 && a);
  CHECK(mem.alloc(&b, 3) == 0 && b);
  CHECK(mem.alloc_host(&h, 16, 0) == 0 && h);
  CHECK(mem.device_bytes() == 80 + 12 && mem.host_bytes() == 64 && mem.live_blocks() == 3);
  check_totals(mem, heap);
  mem.release(a);
  CHECK(mem.device_bytes() == 12);
  mem.release(a);        // a second time: not a live block any more
  mem.release(nullptr);  // null
  int on_stack = 0;
  mem.release(&on_stack);  // never one of its blocks
  check_totals(mem, heap);
  CHECK(mem.live_blocks() == 2);
  mem.release(h);  // a pinned block leaves the device total alone
  CHECK(mem.device_bytes() == 12 && mem.host_bytes() == 0);
  // a failed allocation: status handed on, pointer null, nothing recorded
  heap.fail_at = heap.calls;
  double dummy = 0;
  double* c = &dummy;
  CHECK(mem.alloc(&c, 5) == kNoMem && c == nullptr);
  check_totals(mem, heap);
  mem.release_all();
  CHECK(mem.live_blocks() == 0 && mem.device_bytes() == 0 && mem.host_bytes() == 0);
  CHECK(heap.device.empty() && heap.host.empty());
  mem.release_all();  // again: nothing left to free
  mem.release(b);     // stale after release_all
  CHECK(heap.device.empty());
}

void test_reserve() {
  Heap heap;
  Mem mem(FakeRaw{&heap});
  unsigned char* p = nullptr;
  size_t cap = 0;
  g_quiesced = 0;
  CHECK(mem.reserve(&cap, (size_t)100, (size_t)129, quiesce, pk::want(&p, 129)) == 0);
  CHECK(p && cap == 129 && g_quiesced == 1 && mem.device_bytes() == 129);
  // need <= cap: no allocation, no quiesce, the same block
  const long calls = heap.calls;
  unsigned char* was = p;
  CHECK(mem.reserve(&cap, (size_t)129, (size_t)999, quiesce, pk::want(&p, 999)) == 0);
  CHECK(mem.reserve(&cap, (size_t)0, (size_t)999, quiesce, pk::want(&p, 999)) == 0);
  CHECK(heap.calls == calls && g_quiesced == 1 && p == was && cap == 129);
  // growth frees the old block: the total is the new block's alone
  CHECK(mem.reserve(&cap, (size_t)130, (size_t)166, quiesce, pk::want(&p, 166)) == 0);
  CHECK(cap == 166 && g_quiesced == 2 && mem.device_bytes() == 166 && mem.live_blocks() == 1);
  check_totals(mem, heap);
  // a failed growth: pointer null, capacity 0, nothing held; the next call allocates again
  heap.fail_at = heap.calls;
  CHECK(mem.reserve(&cap, (size_t)200, (size_t)254, quiesce, pk::want(&p, 254)) == kNoMem);
  CHECK(p == nullptr && cap == 0 && mem.device_bytes() == 0 && mem.live_blocks() == 0);
  CHECK(mem.reserve(&cap, (size_t)200, (size_t)254, quiesce, pk::want(&p, 254)) == 0);
  CHECK(p && cap == 254 && mem.device_bytes() == 254);
  // a quiesce that fails: its status comes back and nothing is touched
  was = p;
  CHECK(mem.reserve(&cap, (size_t)300, (size_t)379, [] { return -2; }, pk::want(&p, 379)) == -2);
  CHECK(p == was && cap == 254 && mem.device_bytes() == 254);
  check_totals(mem, heap);
}

// three buffers of different types and sizes behind one capacity; the k-th of the three allocations fails
void test_group_reserve() {
  for (int k = 0; k < 3; ++k) {
    Heap heap;
    Mem mem(FakeRaw{&heap});
    double* a = nullptr;
    int64_t* b = nullptr;
    unsigned* c = nullptr;
    int64_t cap = 0;
    auto grow = [&](int64_t need) {
      return mem.reserve(&cap, need, need + need / 4, quiesce, pk::want(&a, (size_t)need), pk::want(&b, (size_t)need + 1),
                         pk::want(&c, 2 * (size_t)need));
    };
    CHECK(grow(8) == 0 && a && b && c && cap == 10);
    CHECK(mem.device_bytes() == 8 * 8 + 9 * 8 + 16 * 4 && mem.live_blocks() == 3);
    heap.fail_at = heap.calls + k;
    CHECK(grow(20) == kNoMem);
    CHECK(cap == 0);
    // every member is null or a live block of the registry: the ones before the failure were allocated, the rest are null
    CHECK((a != nullptr) == (k > 0) && (b != nullptr) == (k > 1) && c == nullptr);
    CHECK(mem.live_blocks() == (size_t)k);
    CHECK(mem.device_bytes() == (k > 0 ? 20 * 8 : 0) + (size_t)(k > 1 ? 21 * 8 : 0));
    if (a) CHECK(heap.device.count(a) == 1);
    if (b) CHECK(heap.device.count(b) == 1);
    check_totals(mem, heap);
    // the retry starts from scratch and leaves one block per member
    CHECK(grow(20) == 0 && a && b && c && cap == 25 && mem.live_blocks() == 3);
    check_totals(mem, heap);
  }
}

// any sequence: the totals are the sums over what is live
void test_random_sequences() {
  Heap heap;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&rng](unsigned n) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((rng >> 33) % n);
  };
  {
    Mem mem(FakeRaw{&heap});
    constexpr int kSlots = 12;
    unsigned char* dev[kSlots] = {nullptr};
    float* host[kSlots] = {nullptr};
    double* grown[kSlots] = {nullptr};
    size_t cap[kSlots] = {0};
    double* ga = nullptr;
    unsigned* gb = nullptr;
    int64_t gcap = 0;
    for (int step = 0; step < 4000; ++step) {
      const int i = (int)next(kSlots);
      if (next(16) == 0) heap.fail_at = heap.calls + next(3);  // now and then an allocation fails
      switch (next(6)) {
        case 0:
          mem.release(dev[i]);
          if (mem.alloc(&dev[i], 1 + next(300))) CHECK(dev[i] == nullptr);
          break;
        case 1:
          mem.release(host[i]);
          if (mem.alloc_host(&host[i], 1 + next(50), 0)) CHECK(host[i] == nullptr);
          break;
        case 2:
          mem.release(dev[i]);
          dev[i] = nullptr;
          break;
        case 3:
          mem.release(host[i]);  // (left dangling on purpose now and then: a second release must do nothing...
          if (next(2)) host[i] = nullptr;
          else if (host[i]) {
            mem.release(host[i]);  // ... as long as no newer block took the address)
            host[i] = nullptr;
          }
          break;
        case 4: {
          const size_t need = next(400);
          const int rc = mem.reserve(&cap[i], need, need + need / 4 + 2, quiesce, pk::want(&grown[i], need + need / 4 + 2));
          CHECK(rc ? (grown[i] == nullptr && cap[i] == 0) : (cap[i] >= need && (need == 0 || grown[i])));
          break;
        }
        default: {
          const int64_t need = next(200);
          const int rc = mem.reserve(&gcap, need, need + 7, quiesce, pk::want(&ga, (size_t)need + 7), pk::want(&gb, 3 * (size_t)need + 1));
          CHECK(rc ? gcap == 0 : (gcap >= need && (need == 0 || (ga && gb))));
          break;
        }
      }
      check_totals(mem, heap);
    }
    CHECK(mem.live_blocks() > 0);
  }  // the registry goes: so does everything it still held
  CHECK(heap.device.empty() && heap.host.empty());
}

}  // namespace

int main() {
  test_alloc_release();
  test_reserve();
  test_group_reserve();
  test_random_sequences();
  std::printf("devmem ok\n");
  return 0;
}
