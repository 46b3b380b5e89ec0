// Host check (tests/test_hostcheck_cpu.py): models.cpp and pack.cpp of the product, linked against HIP stand-ins backed by host
// memory and launch auditors instead of the kernels.  No HIP runtime, no Python: the program cannot open a GPU.
#pragma once
#include <cstddef>
#include <string>

namespace ss4k { struct Model; }

namespace hc {

// registry of live "device" allocations (base, requested bytes)
void* reg_alloc(size_t bytes);
void reg_free(void* p);
size_t reg_live();
// positive control: the registry forgets the last `bytes` bytes of the allocation that starts at `base` (the memory itself stays)
void reg_shrink(const void* base, size_t bytes);
// is [p, p + bytes) inside ONE live allocation?  (bytes == 0: yes)
bool reg_inside(const void* p, size_t bytes, size_t* off, size_t* alloc_bytes);

// where the walk is: printed with every violation
struct Where {
  std::string desc, shape;
  const ss4k::Model* model = nullptr;
  int launch = 0;          // launches of the current forward so far (conv, pair, dense, glue and FSRCNN alike)
};
extern Where g_where;
extern long g_violations, g_launches;
extern bool g_trace;   // --trace: one line per launch (kind, layer, whether the layer carries a w16 blob)

}  // namespace hc
