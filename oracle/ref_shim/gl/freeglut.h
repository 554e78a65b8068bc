// Stand-in of this repository for freeglut (TEST INFRASTRUCTURE): names that let the reference's window code compile; never called.
#pragma once
enum { GLUT_RGB = 0, GLUT_DOUBLE = 2, GLUT_DEPTH = 16, GLUT_LEFT_BUTTON = 0, GLUT_DOWN = 0, GLUT_UP = 1 };
inline void glutInit(int*, char**) {}
inline void glutInitDisplayMode(unsigned) {}
inline void glutInitWindowSize(int, int) {}
inline void glutInitWindowPosition(int, int) {}
inline int glutCreateWindow(const char*) { return 0; }
inline void glutKeyboardFunc(void (*)(unsigned char, int, int)) {}
inline void glutDisplayFunc(void (*)(void)) {}
inline void glutReshapeFunc(void (*)(int, int)) {}
inline void glutMouseFunc(void (*)(int, int, int, int)) {}
inline void glutIdleFunc(void (*)(void)) {}
inline void glutMainLoop() {}
inline void glutPostRedisplay() {}
inline void glutSwapBuffers() {}
inline void glutReshapeWindow(int, int) {}
