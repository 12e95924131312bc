// esl_graph_int.hpp — what esl_graph.hip (graph residency) and esl_capi.hip (context, launches, LM drivers) share
#pragma once
#include "esl_ctx.hpp"

namespace esl {
template <class T>
static void dev_free(T** p) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
}
// grow-only device blob: kept while it holds `need` bytes, replaced by one half as large again otherwise
int arena_reserve(char** dev, size_t* cap, size_t need);
// sizes, non-null arrays and index ranges of a caller's graph (ESL_ERR_INVALID + the error text)
int validate_graph(const esl_graph* g);
// the resident graph goes away: interior pointers of the arenas are forgotten, the arenas stay
void free_graph(esl_ctx* c);
// The work buffers of a graph with room for this many ellipsoids, cameras and chunks (an upload passes its exact counts, the
// appendable layout its capacities) out of the context's work arena, obj_part zeroed.  In esl_capi.hip beside the launches:
// the sizes are set by kernel headers esl_graph.hip does not include.
int work_buffers(esl_ctx* c, size_t cap_objs, size_t cap_cams, size_t cap_chunks);
}  // namespace esl
