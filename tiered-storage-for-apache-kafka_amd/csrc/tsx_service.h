// The compressor service, host side, as the front end (tsx_api.hip, tsx_batch.hip) sees it: a device's service is created with the device, batches that
// compress become its members, everything that frees memory or runs ordinary kernels tells it.  What is inside tsx_service - the queue,
// the launches, their timing - is tsx_service.hip's alone.  (Also there: tsx_service_quiesce, tsx_service_stats, tsx_debug_service_seed.)
#pragma once
#include "tsx_host.h"

// A batch that has waited this long for its own kernels while the service kernel is alive asks that launch to end (svc_rotate)
#define SVC_ROTATE_AFTER_MS 200

int svc_create(tsx_device& d, int cus);                     // (device current) queue, device words, CU probe, reservation, measured residency
void svc_destroy(tsx_device& d);

struct svc_geometry { uint32_t waves, cus_reserved, cus; }; // waves of a launch; compute units left to fetches, of how many
svc_geometry svc_geometry_of(const tsx_device& d);

// A batch of ordinary kernels begins / is over (no lock: this is the fetch path).  traffic = false: something that only needed room while it
// ran (a new context's first small copies, a helper copy) - it does not count as a fetch having been seen: the device is as quiet afterwards
// as it was before
void svc_foreground_begin(tsx_device* dev);
void svc_foreground_end(tsx_device* dev, bool traffic = true);
struct svc_foreground_scope {                               // begin ... end(dev) around a scope; dev == nullptr: nothing is claimed
    tsx_device* d;
    explicit svc_foreground_scope(tsx_device* dev) : d(dev) { if (d) svc_foreground_begin(d); }
    ~svc_foreground_scope() { if (d) svc_foreground_end(d); }
    svc_foreground_scope(const svc_foreground_scope&) = delete;
    svc_foreground_scope& operator=(const svc_foreground_scope&) = delete;
};

// Is the launch out, or are members waiting for one?  (What launch_stages asks before a decode that would need scratch.)
bool svc_busy(tsx_device* dev);

// Frees that must not wait for the service kernel: at once when it is known to be gone, otherwise when its end is seen or at shutdown
void svc_free_dev(tsx_device* dev, void* p);
void svc_free_host(tsx_device* dev, void* p);
// Memory management that needs the memory BACK: no launches between the two; svc_pause returns when nothing of the service is alive
void svc_pause(tsx_device* dev);
void svc_resume(tsx_device* dev);
// The safety net of the fetch side: asks the running launch to end
void svc_rotate(tsx_device* dev);

// Members: publish (the id is for svc_retire), wait for the member's flag, retire (completed or abandoned)
int svc_submit(tsx_device* dev, const tsx_zseg& proto, const uint32_t* h_flag, uint64_t* id);
int svc_wait(tsx_device* dev, uint32_t* h_flag);
void svc_retire(tsx_device* dev, uint64_t id, bool abandon);
