// vrc_ipc.cpp -- the cross-process side of the C ABI (include/vrc.h): opening a peer's exported framebuffer, and the frame
// flags in shared memory with their watchdog.  Needs no renderer.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "vrc_host.h"

// ---- direct peer writes ("... or direct peer writes into the root's framebuffer") ----
// The presenting rank exports its renderer's framebuffer; every other rank opens it and makes it the target of its own
// renderer, whose frame kernel then writes this rank's rows of the frame where they belong: no pack, no collective, no
// unpack.  Ordering across processes is by interprocess events (one per frame slot and direction).
static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(vrc_ipc_handle), "vrc_ipc_handle too small for hipIpcMemHandle_t");

extern "C" int vrc_ipc_open_image(int device, const vrc_ipc_handle* handle, void** image_dev)
{
    if (!handle || !image_dev) return fail(VRC_ERR_INVALID, "vrc_ipc_open_image: null argument");
    int rc = vrc::require_device(device, nullptr);
    if (rc) return rc;
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    HIP_TRY(hipIpcOpenMemHandle(image_dev, h, hipIpcMemLazyEnablePeerAccess));
    return VRC_OK;
}

extern "C" int vrc_ipc_close_image(int device, void* image_dev)
{
    if (!image_dev) return VRC_OK;
    int rc = vrc::require_device(device, nullptr);
    if (rc) return rc;
    HIP_TRY(hipIpcCloseMemHandle(image_dev));
    return VRC_OK;
}

// Frame flags shared by the processes of a node: 32-bit counters in a POSIX shared-memory segment that every process maps
// and registers with its HIP runtime, written and waited for IN STREAM ORDER (hipStreamWriteValue32 / hipStreamWaitValue32,
// greater-or-equal): "rank k's rows of frame n are in framebuffer s", "framebuffer s has been consumed up to frame n".  A
// wait names a VALUE, not an earlier call, so the processes need no host messages to keep their calls in order (interprocess
// HIP events would: a wait refers to the last record the waiting process has seen -- and ROCm 7.2's lose count after 32
// records per event).
struct vrc_ipc_flags {
    int device = 0;
    uint32_t count = 0;
    size_t bytes = 0;
    uint32_t* host = nullptr;     // the mapping
    uint32_t* dev = nullptr;      // the same words as the device sees them
    bool owner = false;
    bool unlinked = false;        // the creator has removed the name already (vrc_ipc_flags_unlink)
    bool drain_failed = false;    // a stream of this process did not drain within the cap after the exchange was given up
    char name[96] = {0};
};
// the segment: `count` flags, then four words of header {magic, owner's pid, count, given up}
constexpr uint32_t VRC_FLAGS_MAGIC = 0x56524346u;   // "VRCF"
enum { FLAGS_HDR_MAGIC = 0, FLAGS_HDR_OWNER = 1, FLAGS_HDR_COUNT = 2, FLAGS_HDR_GIVEN_UP = 3, FLAGS_HDR_WORDS = 4 };

static bool process_gone(int32_t pid)
{
    if (pid <= 0) return false;
    if (kill((pid_t)pid, 0) != 0 && errno == ESRCH) return true;
    // a child that exited but has not been reaped still has a pid: its state in /proc/<pid>/stat is Z
    char path[64], buf[512];
    snprintf(path, sizeof(path), "/proc/%d/stat", (int)pid);
    FILE* fp = fopen(path, "r");
    if (!fp) return false;
    const size_t n = fread(buf, 1, sizeof(buf) - 1, fp);
    fclose(fp);
    buf[n] = 0;
    const char* rp = strrchr(buf, ')');                        // "pid (comm) S ..."
    return rp && rp[1] == ' ' && (rp[2] == 'Z' || rp[2] == 'X');
}

extern "C" int vrc_ipc_flags_open(const char* name, uint32_t count, int device, int create, vrc_ipc_flags** out)
{
    if (!name || !out || !count || count > (1u << 20)) return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: bad argument");
    if (name[0] != '/' || strlen(name) >= sizeof(vrc_ipc_flags::name)) return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: name must be \"/something\" (shm_open)");
    int rc = vrc::require_device(device, nullptr);
    if (rc) return rc;
    const size_t page = 4096, bytes = (((size_t)(count + FLAGS_HDR_WORDS) * 4u) + page - 1) / page * page;
    int fd = create ? shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600) : shm_open(name, O_RDWR, 0600);
    if (fd < 0 && create && errno == EEXIST) {
        // a segment of that name exists: replace it only when the process that made it is gone (a run that died) -- unlinking
        // one that is in use would leave its processes waiting on memory nobody else maps
        int32_t owner_pid = 0;
        const int old = shm_open(name, O_RDONLY, 0600);
        if (old >= 0) {
            struct stat sb;
            if (fstat(old, &sb) == 0 && sb.st_size >= (off_t)(FLAGS_HDR_WORDS * 4)) {
                // the header sits behind the flags; its count word says where
                void* m0 = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_SHARED, old, 0);
                if (m0 != MAP_FAILED) {
                    const uint32_t* w = (const uint32_t*)m0;
                    const size_t words = (size_t)sb.st_size / 4u;
                    for (size_t c = 0; c + FLAGS_HDR_WORDS <= words; ++c)        // find {magic, pid, count == c}
                        if (w[c + FLAGS_HDR_MAGIC] == VRC_FLAGS_MAGIC && w[c + FLAGS_HDR_COUNT] == (uint32_t)c) { owner_pid = (int32_t)w[c + FLAGS_HDR_OWNER]; break; }
                    munmap(m0, (size_t)sb.st_size);
                }
            }
            close(old);
        }
        if (owner_pid > 0 && owner_pid != (int32_t)getpid() && !process_gone(owner_pid))
            return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: %s is in use by process %d (give concurrent runs different names)", name, (int)owner_pid);
        shm_unlink(name);
        fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
    }
    if (fd < 0) return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: shm_open(%s): %s", name, strerror(errno));
    if (create && ftruncate(fd, (off_t)bytes) != 0) {           // a new segment reads as zeros
        const int e = errno; close(fd); shm_unlink(name);
        return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: ftruncate: %s", strerror(e));
    }
    if (!create) {                                               // never map past what is there: that is a SIGBUS on first touch
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size < (off_t)bytes) {
            close(fd);
            return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: %s holds %lld bytes, %u flags need %zu (not created yet, or made for another count)",
                        name, (long long)sb.st_size, count, bytes);
        }
    }
    void* m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    const int em = errno;
    close(fd);
    if (m == MAP_FAILED) { if (create) shm_unlink(name); return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: mmap: %s", strerror(em)); }
    hipError_t e = hipHostRegister(m, bytes, hipHostRegisterMapped);
    void* d = nullptr;
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, m, 0);
    if (e != hipSuccess) {
        munmap(m, bytes);
        if (create) shm_unlink(name);
        return fail(VRC_ERR_HIP, "vrc_ipc_flags_open: registering the segment: %s", hipGetErrorString(e));
    }
    uint32_t* hdr = (uint32_t*)m + count;
    if (create) {
        hdr[FLAGS_HDR_OWNER] = (uint32_t)getpid(); hdr[FLAGS_HDR_COUNT] = count; hdr[FLAGS_HDR_GIVEN_UP] = 0u;
        __atomic_store_n(hdr + FLAGS_HDR_MAGIC, VRC_FLAGS_MAGIC, __ATOMIC_RELEASE);
    } else if (__atomic_load_n(hdr + FLAGS_HDR_MAGIC, __ATOMIC_ACQUIRE) != VRC_FLAGS_MAGIC || hdr[FLAGS_HDR_COUNT] != count) {
        (void)hipHostUnregister(m);
        munmap(m, bytes);
        return fail(VRC_ERR_INVALID, "vrc_ipc_flags_open: %s was not made for %u flags", name, count);
    }
    vrc_ipc_flags* f = new vrc_ipc_flags;
    f->device = device; f->count = count; f->bytes = bytes; f->host = (uint32_t*)m; f->dev = (uint32_t*)d; f->owner = create != 0;
    snprintf(f->name, sizeof(f->name), "%s", name);
    *out = f;
    return VRC_OK;
}

static bool flags_given_up(const vrc_ipc_flags* f) { return __atomic_load_n(f->host + f->count + FLAGS_HDR_GIVEN_UP, __ATOMIC_ACQUIRE) != 0u; }

// the watchdog of a stream that waits for flags (include/vrc.h).  timeout_ms is an INACTIVITY limit: the clock starts again
// whenever any flag of the segment changes (a frame of some rank completed), so a healthy exchange that is still draining a
// long queue is never declared dead -- only one on which nothing has moved for timeout_ms.
extern "C" int vrc_ipc_stream_wait(vrc_ipc_flags* f, void* stream, const int32_t* pids, uint32_t n_pids, uint32_t timeout_ms)
{
    if (!f || (n_pids && !pids)) return fail(VRC_ERR_INVALID, "vrc_ipc_stream_wait: bad argument");
    HIP_TRY(hipSetDevice(f->device));
    auto flags_digest = [f]() {                                    // changes whenever a flag does (flags only ever grow)
        uint64_t d = 0;
        for (uint32_t i = 0; i < f->count; ++i) d += __atomic_load_n(f->host + i, __ATOMIC_RELAXED);
        return d;
    };
    const auto t_begin = std::chrono::steady_clock::now();
    auto t_progress = t_begin;
    uint64_t digest = flags_digest();
    const char* why = nullptr;
    int32_t who = 0;
    uint32_t polls = 0;
    for (;;) {
        const hipError_t q = hipStreamQuery((hipStream_t)stream);
        if (q == hipSuccess) return flags_given_up(f) ? fail(VRC_ERR_PEER, "vrc_ipc_stream_wait: the exchange was given up (a peer died or timed out)") : VRC_OK;
        if (q != hipErrorNotReady) return fail(VRC_ERR_HIP, "vrc_ipc_stream_wait: hipStreamQuery: %s", hipGetErrorString(q));
        if (flags_given_up(f)) { why = "another process gave the exchange up"; break; }
        const auto now = std::chrono::steady_clock::now();
        const long long us = std::chrono::duration_cast<std::chrono::microseconds>(now - t_begin).count();
        // the caller usually sits in a timed region: the first 3 ms are polled without sleeping (a stream that is nearly
        // drained ends within a poll, not within a sleep), then 50 us naps, 500 us ones after 100 ms.  The peers and the
        // flags are looked at every 64th poll (every few milliseconds once the naps have begun), as before
        if ((++polls & 63u) == 0u) {
            const uint64_t d = flags_digest();
            if (d != digest) { digest = d; t_progress = now; }
            for (uint32_t k = 0; k < n_pids && !why; ++k)
                if (process_gone(pids[k])) { why = "a peer process is gone"; who = pids[k]; }
            if (why) break;
            const auto idle_ms = std::chrono::duration_cast<std::chrono::milliseconds>(now - t_progress).count();
            if (timeout_ms && idle_ms >= (long long)timeout_ms) { why = "no flag moved within the timeout"; break; }
        }
        if (us >= 3000) std::this_thread::sleep_for(std::chrono::microseconds(us < 100000 ? 50 : 500));
    }
    // give up for everyone: mark the segment, then release every wait on its flags (>= comparisons: the largest value passes all).
    // The release has to be HELD while the stream drains: the stream-ordered flag writes still queued behind the waits (this
    // process's and the peers') put ordinary frame numbers back into the flags, and a wait that comes after such a write would
    // block again -- so the flags are re-asserted until this stream is empty (every process's own watchdog does the same for its
    // stream; bounded, in case the device itself is gone).
    __atomic_store_n(f->host + f->count + FLAGS_HDR_GIVEN_UP, 1u, __ATOMIC_RELEASE);
    const auto t1 = std::chrono::steady_clock::now();
    // (bounded: 20 s for the first stream of this process that does not drain -- the device itself may be gone, or busy tearing
    // the dead process down --, 2 s for every one after it, so that a process with several streams still leaves within half a minute)
    const long long cap_ms = f->drain_failed ? 2000 : 20000;
    bool drained = false;
    for (;;) {
        for (uint32_t i = 0; i < f->count; ++i) __atomic_store_n(f->host + i, 0xffffffffu, __ATOMIC_RELEASE);
        if (hipStreamQuery((hipStream_t)stream) != hipErrorNotReady) { drained = true; break; }
        if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t1).count() >= cap_ms) break;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    if (!drained) f->drain_failed = true;
    // once more behind the last operation of this stream: a flag write that was still queued may have landed after the last
    // store above and put an ordinary frame number back, on which another process's later wait would block again
    for (uint32_t i = 0; i < f->count; ++i) __atomic_store_n(f->host + i, 0xffffffffu, __ATOMIC_RELEASE);
    return fail(VRC_ERR_PEER, "vrc_ipc_stream_wait: %s (pid %d); every wait on %s was released, frames after this are not valid", why, (int)who, f->name);
}

// Once every process of the run has opened the segment its NAME is no longer needed: the creator removes it (the mappings stay
// valid until the last process unmaps), so a run that is killed later leaves nothing behind in /dev/shm.
extern "C" int vrc_ipc_flags_unlink(vrc_ipc_flags* f)
{
    if (!f) return fail(VRC_ERR_INVALID, "vrc_ipc_flags_unlink: null argument");
    if (!f->owner) return fail(VRC_ERR_INVALID, "vrc_ipc_flags_unlink: only the process that created %s removes its name", f->name);
    if (!f->unlinked && shm_unlink(f->name) != 0 && errno != ENOENT)
        return fail(VRC_ERR_INVALID, "vrc_ipc_flags_unlink: shm_unlink(%s): %s", f->name, strerror(errno));
    f->unlinked = true;
    return VRC_OK;
}

extern "C" int vrc_ipc_flags_close(vrc_ipc_flags* f)
{
    if (!f) return VRC_OK;
    (void)hipSetDevice(f->device);
    (void)hipHostUnregister(f->host);
    munmap(f->host, f->bytes);
    if (f->owner && !f->unlinked) shm_unlink(f->name);
    delete f;
    return VRC_OK;
}

extern "C" int vrc_stream_write_flag(vrc_ipc_flags* f, uint32_t index, uint32_t value, void* stream)
{
    if (!f || index >= f->count) return fail(VRC_ERR_INVALID, "vrc_stream_write_flag: bad argument");
    if (flags_given_up(f)) return fail(VRC_ERR_PEER, "vrc_stream_write_flag: the exchange on %s was given up", f->name);
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipStreamWriteValue32((hipStream_t)stream, f->dev + index, value, 0));
    return VRC_OK;
}

extern "C" int vrc_stream_wait_flag(vrc_ipc_flags* f, uint32_t index, uint32_t value, void* stream)
{
    if (!f || index >= f->count) return fail(VRC_ERR_INVALID, "vrc_stream_wait_flag: bad argument");
    if (flags_given_up(f)) return fail(VRC_ERR_PEER, "vrc_stream_wait_flag: the exchange on %s was given up", f->name);
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipStreamWaitValue32((hipStream_t)stream, f->dev + index, value, hipStreamWaitValueGte, 0xffffffffu));
    return VRC_OK;
}

extern "C" int vrc_ipc_flag_set(vrc_ipc_flags* f, uint32_t index, uint32_t value)
{
    if (!f || index >= f->count) return fail(VRC_ERR_INVALID, "vrc_ipc_flag_set: bad argument");
    __atomic_store_n(f->host + index, value, __ATOMIC_RELEASE);
    return VRC_OK;
}

extern "C" uint32_t vrc_ipc_flag_value(const vrc_ipc_flags* f, uint32_t index)
{
    return (f && index < f->count) ? __atomic_load_n(f->host + index, __ATOMIC_ACQUIRE) : 0u;
}
