// Stand-in of this repository for GLEW (TEST INFRASTRUCTURE): names that let the reference's window code compile; never called.
#pragma once
typedef unsigned int GLuint;
typedef unsigned int GLenum;
typedef int GLsizei;
typedef int GLint;
typedef float GLclampf;
enum {
    GL_PIXEL_UNPACK_BUFFER_ARB = 0x88EC, GL_DYNAMIC_DRAW_ARB = 0x88E8, GL_COLOR_BUFFER_BIT = 0x4000, GL_RGBA = 0x1908,
    GL_UNSIGNED_BYTE = 0x1401, GL_BGR = 0x80E0
};
inline int glewInit() { return 0; }
inline void glGenBuffers(GLsizei, GLuint*) {}
inline void glBindBuffer(GLenum, GLuint) {}
inline void glBufferData(GLenum, long, const void*, GLenum) {}
inline void glDeleteBuffers(GLsizei, const GLuint*) {}
inline void glClearColor(GLclampf, GLclampf, GLclampf, GLclampf) {}
inline void glClear(unsigned) {}
inline void glDrawPixels(GLsizei, GLsizei, GLenum, GLenum, const void*) {}
inline void glReadPixels(GLint, GLint, GLsizei, GLsizei, GLenum, GLenum, void*) {}
