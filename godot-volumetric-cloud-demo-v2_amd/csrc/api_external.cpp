// api_external.cpp -- zero-copy interop: a frame that lives in memory another API allocated (csky_external_frame_*, cloudsky.h;
// gdext/unverified/zero_copy_vulkan.c is the Vulkan half).
#include <cerrno>
#include <cstring>
#include <new>
#include <unistd.h>
#include <sys/syscall.h>
#include "context.h"

using namespace csky;

struct csky_external_frame { int device = 0; hipExternalMemory_t mem = nullptr; void* d_ptr = nullptr; size_t bytes = 0; hipExternalSemaphore_t sem = nullptr; hipEvent_t fence = nullptr; bool fenced = false; };

namespace {

// Does descriptor `a` still name the open file description that `b` names?  1 yes, 0 no, -1 cannot tell.  kcmp(KCMP_FILE) compares the kernel objects
// themselves (device + inode identity is the same for EVERY dma-buf / anon-inode descriptor on kernels that share one anon inode, so it cannot
// tell "ours" from a foreign descriptor that reused the number); where the kernel has no kcmp the answer is "cannot tell".
int same_open_file(int a, int b) {
#ifdef SYS_kcmp
    const long r = syscall(SYS_kcmp, (long)getpid(), (long)getpid(), 0L /* KCMP_FILE */, (long)a, (long)b);
    if (r == 0) return 1;
    if (r > 0) return 0;
    if (errno == EBADF) return 0;                            // `a` is closed: whoever was handed the number consumed it
#endif
    return -1;
}

}  // namespace

extern "C" {

int csky_external_frame_import_fd(csky_ctx* c, int opaque_fd, size_t allocation_bytes, size_t offset, size_t frame_bytes, csky_external_frame** out, void** d_ptr) {
    if (!c || !out || !d_ptr) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_import_fd: NULL argument");
    *out = nullptr; *d_ptr = nullptr;
    if (opaque_fd < 0 || frame_bytes == 0 || frame_bytes > allocation_bytes || offset > allocation_bytes - frame_bytes) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_import_fd: bad fd / sizes");
    int rc; if ((rc = bind(c))) return rc;
    csky_external_frame* f = new (std::nothrow) csky_external_frame();
    if (!f) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_import_fd: out of host memory");
    f->device = c->device; f->bytes = frame_bytes;
    hipExternalMemoryHandleDesc md; memset(&md, 0, sizeof md);
    // The runtime takes ownership of the fd it is given on success and says nothing about failure, so it gets a DUPLICATE: on ANY failure the
    // caller still owns opaque_fd (and only it); on success the library closes the caller's fd, as documented.
    const int dfd = dup(opaque_fd);
    if (dfd < 0) { delete f; return fail(c, CSKY_ERR_INVALID, "csky_external_frame_import_fd: dup(fd) failed"); }
    md.type = hipExternalMemoryHandleTypeOpaqueFd; md.handle.fd = dfd; md.size = allocation_bytes;
    hipError_t e = hipImportExternalMemory(&f->mem, &md);
    if (e != hipSuccess) (void)close(dfd);
    else {
        // Who owns the duplicate now is decided HERE, once, and the number is never looked at again (a later descriptor -- of this process, the engine
        // or the Vulkan driver -- may reuse it).  CUDA's convention: the runtime consumed it at import.  ROCm's CLR maps the dma-buf during the call
        // and does not say; a runtime that keeps neither the number nor closes it would leak one descriptor per imported frame.  So: if the number
        // provably still names OUR open file description (same kernel object as the caller's descriptor, which nobody else can have closed), the
        // runtime did not consume it and the mapping no longer needs it: close it now.  "No" or "cannot tell" (no kcmp in this kernel): leave it --
        // leaking a descriptor is the safe side of closing a foreign one.
        if (same_open_file(dfd, opaque_fd) == 1) (void)close(dfd);
    }
    if (e == hipSuccess) {
        hipExternalMemoryBufferDesc bd; memset(&bd, 0, sizeof bd);
        bd.offset = offset; bd.size = frame_bytes;
        e = hipExternalMemoryGetMappedBuffer(&f->d_ptr, f->mem, &bd);
    }
    if (e != hipSuccess) { csky_external_frame_release(f); return fail(c, CSKY_ERR_HIP, "csky_external_frame_import_fd: %s", hipGetErrorString(e)); }
    (void)close(opaque_fd);                                   // success: the library owns the memory object now
    *out = f; *d_ptr = f->d_ptr;
    return CSKY_OK;
}
int csky_external_frame_import_semaphore_fd(csky_ctx* c, csky_external_frame* f, int opaque_fd) {
    if (!c || !f || opaque_fd < 0) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_import_semaphore_fd: bad argument");
    int rc; if ((rc = bind(c))) return rc;
    if (f->sem) { (void)hipDestroyExternalSemaphore(f->sem); f->sem = nullptr; }
    hipExternalSemaphoreHandleDesc sd; memset(&sd, 0, sizeof sd);
    sd.type = hipExternalSemaphoreHandleTypeOpaqueFd; sd.handle.fd = opaque_fd;
    HIPCHK(c, hipImportExternalSemaphore(&f->sem, &sd));
    return CSKY_OK;
}
int csky_external_frame_signal(csky_ctx* c, csky_external_frame* f, void* hip_stream) {
    if (!c || !f || !f->sem) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_signal: no semaphore imported");
    int rc; if ((rc = bind(c))) return rc;
    hipExternalSemaphoreSignalParams sp; memset(&sp, 0, sizeof sp);
    HIPCHK(c, hipSignalExternalSemaphoresAsync(&f->sem, &sp, 1, hip_stream ? (hipStream_t)hip_stream : c->stream));
    return CSKY_OK;
}
// Host-side ordering for runtimes that cannot import a semaphore (ROCm 7.2 on Linux answers hipErrorNotSupported for every handle type,
// profiles/r03/external_semaphore_probe.txt): an event behind the march that the host polls before it lets the engine sample the image.
int csky_external_frame_fence(csky_ctx* c, csky_external_frame* f, void* hip_stream) {
    if (!c || !f) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_fence: NULL argument");
    int rc; if ((rc = bind(c))) return rc;
    if (!f->fence) HIPCHK(c, hipEventCreateWithFlags(&f->fence, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(f->fence, hip_stream ? (hipStream_t)hip_stream : c->stream));
    f->fenced = true;
    return CSKY_OK;
}
int csky_external_frame_ready(csky_ctx* c, csky_external_frame* f) {
    if (!c || !f) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_ready: NULL argument");
    if (!f->fenced) return fail(c, CSKY_ERR_STATE, "csky_external_frame_ready: no fence recorded (csky_external_frame_fence)");
    const hipError_t e = hipEventQuery(f->fence);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    return fail(c, CSKY_ERR_HIP, "csky_external_frame_ready: %s", hipGetErrorString(e));
}
int csky_external_frame_wait(csky_ctx* c, csky_external_frame* f) {
    if (!c || !f) return fail(c, CSKY_ERR_INVALID, "csky_external_frame_wait: NULL argument");
    if (!f->fenced) return fail(c, CSKY_ERR_STATE, "csky_external_frame_wait: no fence recorded (csky_external_frame_fence)");
    int rc; if ((rc = bind(c))) return rc;
    HIPCHK(c, hipEventSynchronize(f->fence));
    return CSKY_OK;
}
void csky_external_frame_release(csky_external_frame* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->fence) { (void)hipEventSynchronize(f->fence); (void)hipEventDestroy(f->fence); }   // never unmap memory a march may still be writing
    if (f->sem) (void)hipDestroyExternalSemaphore(f->sem);
    if (f->mem) (void)hipDestroyExternalMemory(f->mem);      // unmaps d_ptr
    // (the duplicate descriptor the runtime was handed was settled at import: csky_external_frame_import_fd)
    delete f;
}

}  // extern "C"
