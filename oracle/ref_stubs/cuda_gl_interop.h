/* cuda_gl_interop.h -- TEST INFRASTRUCTURE: the two type names of the CUDA / OpenGL interop API that a translation unit's globals may mention; nothing else. */
#ifndef RT_STUB_CUDA_GL_INTEROP_H
#define RT_STUB_CUDA_GL_INTEROP_H
typedef unsigned int GLuint;
struct cudaGraphicsResource;
#endif
