// Renderer.hpp -- host mirror of the reference's Renderer namespace (Renderer.hpp:1-46): device
// init, instance table, per-frame launch. GL/window parts are gone (headless); Render() returns a
// frame counter instead of a GL texture id and MapOutput() exposes the HDR float4 frame.
#pragma once
#include "ResourceManager.hpp"

typedef CrtMeshInstance MeshInstance;
typedef uint MeshInstanceHandle;

namespace Renderer
{
    constexpr uint MaxNumInstances = 401;

    // device: HIP ordinal; width/height: initial frame (the reference takes them from the window)
    int Initialize(int device = 0, int width = 1249, int height = 720);
    // several GPUs in this process (extension: upstream drives one device): same API afterwards, Render() delivers the
    // whole frame; `devices` lists HIP ordinals (a GPU may be named twice to rehearse the path on a one-GPU box)
    int InitializeDevices(const int* devices, int numDevices, int width = 1249, int height = 720);
    void Terminate();
    // one frame: RayGen -> Trace -> PostProcess -> wait (Renderer.cpp:305-375). Returns the frame
    // index (>0) or 0 on failure (see LastError()).
    unsigned Render(float sunAngle);
    void OnWindowResize(int width, int height);

    void BeginInstanceRegister();
    MeshInstanceHandle RegisterMeshInstance(MeshHandle handle, MaterialHandle material, const Matrix4& mat);
    MeshInstanceHandle RegisterMeshInstance(MeshHandle handle, MaterialHandle material, float3 position, const Quaternion& rotation, const float3& scale);
    void EndInstanceRegister();
    void RemoveMeshInstance(MeshInstanceHandle handle);
    void ClearAllInstances();

    void SetMeshInstanceMaterial(MeshInstanceHandle meshHandle, MaterialHandle materialHandle);
    void SetMeshPosition(MeshInstanceHandle handle, float3 position);
    void SetMeshMatrix(MeshInstanceHandle handle, const Matrix4& matrix);
    const Camera& GetCamera();

    // ---- additions for the headless build ----
    Camera& EditCamera();                 // set position/Front, then RecalculateView()
    void SetPostProcess(bool enabled);    // PostProcess is on upstream; parity is judged pre-post
    void SetUnorm8(bool enabled);         // quantise like upstream's RGBA8 render target (hazard H8); MapOutputRGBA8() returns the bytes
    const unsigned char* MapOutputRGBA8();
    void SetShadows(bool enabled);        // extension: the shadow ray upstream leaves as a TODO (kernel_main.cl:256-258); off by default
    void SetFXAA(bool enabled);           // extension: upstream's FXAA (kernel_main.cl:289-340) is dead code (call commented out, kernel_main.cl:349); runs it as the first PostProcess stage; off by default
    void SetSupersampling(int factor);    // extension: k x k supersampled anti-aliasing resolved in the Trace kernel, factor 1 (default), 2 or 4; any other value sets LastError() to CRT_E_BAD_ARGUMENT and keeps the setting
    void SetGBuffer(bool enabled);        // extension: Render() also writes the first-hit planes (CRT_RENDER_GBUFFER: normal + distance, instance / triangle / barycentrics, albedo); off by default
    const void* MapGBuffer(int plane);    // host copy of plane CRT_GBUFFER_GEOMETRY / IDS / ALBEDO of the last G-buffer frame (width*height elements), valid until next Render; null without one
    bool PickPixel(int x, int y, CrtGBufferPixel& out); // what that frame's primary ray hit at pixel (x, y): 36 bytes from the device, no ray cast (replaces CPU_RayCast(ScreenPointToRaySSE(mouse)), Engine.cpp:112-126)
    // extension: closest hit (CRT_RAYS_CLOSEST: CrtRayHit per ray) or occlusion (CRT_RAYS_OCCLUDED: one byte per ray) for a batch of rays on the device
    // against the registered instances (as last uploaded), enqueued on `stream` (a hipStream_t; null: HIP's null stream) without waiting; false: LastError().
    // mode | CRT_RAYS_INCLUSIVE: the inclusive box test, for rays that start on a surface (crt_api.h)
    bool TraceRays(const CrtRayBatch& rays, int mode, void* out, void* stream = nullptr);
    // extension: what a frame computes for a pixel, for a batch of rays on the device (crt_api.h: crt_shade_rays): `radiance` (float4 per ray) and / or
    // `surface` (the first hit's CrtSurfaceHit per ray) on the device, either may be null; enqueued on `stream` without waiting; false: LastError().
    bool ShadeRays(const CrtRayBatch& rays, const CrtShadeParams& params, float* radiance, CrtSurfaceHit* surface, void* stream = nullptr);
    // extension: ambient occlusion (crt_api.h: crt_trace_ao, crt_frame_ao). TraceAmbientOcclusion: n floats into `out` for points + normals on the device,
    // against the registered instances, enqueued on `stream` without waiting. ComputeAmbientOcclusion: the same for the pixels of the last frame rendered
    // with SetGBuffer(true), into that frame's AO plane; MapAmbientOcclusion: a host copy of it (width*height floats, valid until the next call; null
    // without one). false / null: LastError(). CRT_AO_INCLUSIVE in params.flags: the sample rays under the inclusive box test, both forms
    bool TraceAmbientOcclusion(const CrtAoPoints& points, const CrtAoParams& params, float* out, void* stream = nullptr);
    bool ComputeAmbientOcclusion(const CrtAoParams& params, void* stream = nullptr);
    const float* MapAmbientOcclusion();
    void SetRefraction(bool enabled);     // extension: upstream's README TODO "refraction / transculency": materials with MTL d < 1 transmit; off by default
    void SetPipelined(bool enabled);      // Render() returns without waiting (frames in flight); MapOutput()/uploads wait. Off by default (upstream clFinish()es)
    void SetTime(float seconds);          // TraceArgs.time (Window::GetTime upstream)
    void SetRowBands(int bandRows, int rank, int nRanks); // multi-GPU image tiling
    const float* MapOutput();             // host copy of the float4 frame (width*height*4), valid until next Render
    float LastFrameMs();                  // HIP-event time of the last frame's kernels
    int LastError();                      // first error since Initialize / ClearError (errors are returned as codes, not exit(0): DESIGN.md 8)
    void ClearError();
}

extern uint g_NumMeshInstances;
extern Matrix4* g_MeshTransforms;
extern MeshInstance* g_MeshInstances;
